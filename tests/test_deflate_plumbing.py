"""CPU-side checks of the plumbing of ``ReadWriter(deflate=...)``: what it refuses, that the host route is the writer of
before — its bytes, its ``repr``, and no import of the new module —, the writer threads on the device route (members
written as they are, the end-of-file marker once at ``finish()``, nothing left after ``abort()``), how a chunk queues
the deflate behind the format call and collects it, and the command line."""
import gzip
import os
import subprocess
import sys

import pytest

from genefuserust_amd import cli, deflate, read_write
from genefuserust_amd.read_write import ReadWriter, WriteResult
from tests import bgzf_members as bm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_read_writer_validates_deflate(tmp_path):
    a, b = str(tmp_path / "a.fq.gz"), str(tmp_path / "b.fq.gz")
    w = ReadWriter(a, b)
    assert w.deflate == "host" and w.compressed_bytes is None
    w = ReadWriter(a, b, deflate="device", compress_level=9)
    assert w.deflate == "device" and w.compressed_bytes == (0, 0) and ReadWriter(a, deflate="device").compressed_bytes == (0,)
    for bad in ("gpu", "", None, True, 1, b"device", "Device"):
        with pytest.raises(ValueError, match="deflate must be 'host' or 'device'"):
            ReadWriter(a, b, deflate=bad)
    # the device route writes BGZF: every output name must end in .gz
    for outs in ((str(tmp_path / "a.fq"),), (a, str(tmp_path / "b.fq")), (str(tmp_path / "a.fq"), b),
                 (str(tmp_path / "a.gz.txt"),)):
        with pytest.raises(ValueError, match="does not end in .gz"):
            ReadWriter(*outs, deflate="device")
        ReadWriter(*outs)                                  # (the host route takes them)
    assert "compress_level`` is not used" in ReadWriter.__doc__
    assert os.listdir(tmp_path) == []                      # nothing was opened


def test_the_host_route_is_the_writer_of_before(tmp_path):
    a, b = str(tmp_path / "a.fq"), str(tmp_path / "b.fq.gz")
    w = ReadWriter(a, b, umi_in_name=True, compress_level=7)
    assert repr(w) == "ReadWriter(out1=%r, out2=%r, umi_in_name=True, compress_level=7)" % (a, b)
    assert repr(ReadWriter(a, b, deflate="host")) == repr(ReadWriter(a, b))
    assert "deflate" in repr(ReadWriter(b, deflate="device"))
    assert w.result() == WriteResult(0, 0, (0, 0), 0) and WriteResult._fields == ("records", "bases", "bytes", "not_written")
    w.open(2)
    blocks = [(b"@r%d\nACGT\n+\nFFFF\n" % k) * (k + 1) for k in range(5)]
    for block in blocks:
        w.hand_over(0, block)
        w.hand_over(1, block)
    w.finish()
    packed = open(b, "rb").read()
    # plain gzip members, one a block, zlib's bytes at the level asked for, and no BGZF marker behind them
    import zlib
    want = b""
    for block in blocks:
        c = zlib.compressobj(7, zlib.DEFLATED, 31)
        want += c.compress(block) + c.flush()
    assert packed == want and not packed.endswith(deflate.EOF_MARKER) and open(a, "rb").read() == b"".join(blocks)


def test_the_host_route_does_not_import_the_new_module(tmp_path):
    code = ("import sys\n"
            "from genefuserust_amd.read_write import ReadWriter\n"
            "w = ReadWriter(%r, %r)\n"
            "w.open(2); w.hand_over(0, b'x'); w.hand_over(1, b'y'); w.finish()\n"
            "assert 'genefuserust_amd.deflate' not in sys.modules\n"
            "w = ReadWriter(%r, deflate='device')\n"
            "assert 'genefuserust_amd.deflate' not in sys.modules\n"      # (not before the files are opened)
            "w.open(1); w.finish()\n"
            "assert 'genefuserust_amd.deflate' in sys.modules\n"
            % (str(tmp_path / "a.fq"), str(tmp_path / "b.fq.gz"), str(tmp_path / "c.fq.gz")))
    done = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert done.returncode == 0, done.stderr


def test_the_device_route_writes_members_as_they_are_and_the_marker_once(tmp_path):
    a, b = str(tmp_path / "a.fq.gz"), str(tmp_path / "b.fq.gz")
    w = ReadWriter(a, b, deflate="device")
    w.open(2)
    texts = [bm.fastq_text(3000 + 500 * k, seed=k + 1) for k in range(6)]       # more blocks than the queue is deep
    released = []
    for k, text in enumerate(texts):
        w.hand_over(0, deflate.deflate_host(text), lambda k=k: released.append(k))
        w.hand_over(1, bytearray(deflate.deflate_member_host(text)))
    w.finish()
    assert sorted(os.listdir(tmp_path)) == ["a.fq.gz", "b.fq.gz"] and sorted(released) == list(range(6))
    for path in (a, b):
        data = open(path, "rb").read()
        assert data == b"".join(deflate.deflate_member_host(t) for t in texts) + deflate.EOF_MARKER
        assert gzip.decompress(data) == b"".join(texts)
        rows, used, total, why, _ = bm.walk_model(data)
        assert why == bm.WALK_END and used == len(data) and [r[3] for r in rows] == [len(t) for t in texts] + [0]
    # a scan that writes no record leaves just the marker
    w = ReadWriter(str(tmp_path / "e.fq.gz"), deflate="device")
    w.open(1)
    w.finish()
    assert open(w.out1, "rb").read() == deflate.EOF_MARKER and gzip.decompress(deflate.EOF_MARKER) == b""
    assert w.compressed_bytes == (0,)


def test_no_file_is_left_after_abort(tmp_path):
    import threading
    threads = threading.active_count()
    w = ReadWriter(str(tmp_path / "a.fq.gz"), str(tmp_path / "b.fq.gz"), deflate="device")
    w.open(2)
    assert sorted(os.listdir(tmp_path)) == ["a.fq.gz.tmp", "b.fq.gz.tmp"]
    w.hand_over(0, deflate.deflate_member_host(b"@r\nACGT\n+\nFFFF\n"))
    w.abort()
    assert os.listdir(tmp_path) == [] and threading.active_count() == threads
    with pytest.raises(ValueError, match="has served a scan"):
        w.open(2)


class _Tensor:
    """As much of a device tensor as ``format_chunk`` and ``collect`` look at."""

    def __init__(self, values, name=""):
        self.values, self.name = list(values), name

    def __getitem__(self, key):
        return _Tensor(self.values[key], self.name + "[%s:%s]" % (key.start, key.stop))

    def numel(self):
        return len(self.values)


def test_a_chunk_queues_the_deflate_behind_the_format_call_on_its_output(monkeypatch, tmp_path):
    calls = []
    out_texts, out_offs = [_Tensor(range(100), "text0"), _Tensor(range(100), "text1")], \
        [_Tensor(range(4), "off0"), _Tensor(range(4), "off1")]

    def format_reads(indexer, texts, cuts, finals, n, **kw):
        calls.append(("format", n))
        return out_texts, out_offs, "totals"

    def deflate_device(text, text_bytes=None, stream=None):
        calls.append(("deflate", text.name, text_bytes.name))
        return ("packed " + text.name, "member_off", "deflate totals")

    class _B:
        offsets = list(range(6))

        def _replace(self, **kw):
            return self
    monkeypatch.setattr(read_write, "format_reads_device", format_reads)
    monkeypatch.setattr(deflate, "deflate_device", deflate_device)
    a, b = str(tmp_path / "a.fq.gz"), str(tmp_path / "b.fq.gz")
    got = ReadWriter(a, b, deflate="device").format_chunk("ix", ["t0", "t1"], ["c0", "c1"], [_B(), _B()], 3)
    # the text's length is the format call's out_off[n], still on the device
    assert calls == [("format", 3), ("deflate", "text0", "off0[3:4]"), ("deflate", "text1", "off1[3:4]")]
    assert got[:3] == (out_texts, out_offs, "totals")
    assert got[3] == [("packed text0", "member_off", "deflate totals"), ("packed text1", "member_off", "deflate totals")]
    del calls[:]
    got = ReadWriter(a, b).format_chunk("ix", ["t0", "t1"], ["c0", "c1"], [_B(), _B()], 3)
    assert calls == [("format", 3)] and got == (out_texts, out_offs, "totals")       # the host route: the call of before


def test_cli_option(tmp_path):
    def args(*extra):
        return cli.parser().parse_args(["-1", "a.fq", "-f", "x.csv", "-r", "ref.fa", *extra])
    a, b = str(tmp_path / "a.fq.gz"), str(tmp_path / "b.fq.gz")
    assert cli._read_writer(args("--out1", a)).deflate == "host"
    assert cli._read_writer(args("--out1", a, "--out-deflate", "host")).deflate == "host"
    w = cli._read_writer(args("--out1", a, "--out2", b, "--out-deflate", "device"))
    assert isinstance(w, ReadWriter) and w.deflate == "device" and w.outputs == (a, b)
    for value in ("host", "device"):
        with pytest.raises(ValueError, match="--out-deflate needs --out1"):
            cli._read_writer(args("--out-deflate", value))
    with pytest.raises(ValueError, match="does not end in .gz"):
        cli._read_writer(args("--out1", str(tmp_path / "a.fq"), "--out-deflate", "device"))
    with pytest.raises(SystemExit):
        args("--out1", a, "--out-deflate", "gpu")
    assert "--out-deflate" in cli.parser().format_help()
    assert os.listdir(tmp_path) == []
