"""The streamed file routes with ``inflate="device"`` on the MI355X: BGZF files inflated on the device against the same
files gunzipped on the host (``inflate="host"``), as whole results and counters, ``chunks`` included; ``"auto"``; and the
errors of files that are not BGZF, that hold a bad member, that are cut."""
import gzip
import os

import pytest

from tests import bgzf_members as bm
from tests.test_multi_csv_scan import _files, _texts
from tests.test_stream_files import _names_of

pytestmark = pytest.mark.gpu
SIZES = (4000, 1, 65280, 1, 4000)     # text bytes of the members, in turn


def _bgzf(path: str, sizes=SIZES) -> str:
    out = path + ".gz"
    text = open(path, "rb").read()
    with open(out, "wb") as f:
        f.write(bm.bgzf(text, sizes))
    assert gzip.open(out, "rb").read() == text
    return out


def _same(device, host):
    (d_res, d_cnt), (h_res, h_cnt) = device, host
    assert d_cnt == h_cnt and "chunks" in h_cnt
    assert _texts(d_res) == _texts(h_res) and _names_of(d_res) == _names_of(h_res)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("inflate_files")
    fa, lst, csvs, r1, r2 = _files(tmp)
    # (the files are longer than one 4000-byte member and one chunk of 4096 bytes by far)
    assert min(os.path.getsize(p) for p in (fa, r1, r2)) > 20000
    return dict(tmp=tmp, fa=fa, lst=lst, csvs=csvs, r1=r1, r2=r2, zfa=_bgzf(fa), z1=_bgzf(r1), z2=_bgzf(r2))


@pytest.mark.parametrize("chunk_bytes", [4096, 65281, 1 << 20])
def test_pair_end_report(gpu_device, files, chunk_bytes):
    from genefuserust_amd.scan import scan_pair_end_report
    f = files
    host = scan_pair_end_report(f["fa"], f["csvs"][3], f["z1"], f["z2"], chunk_bytes=chunk_bytes, inflate="host")
    assert host[1]["fusions"] >= 1 and host[1]["pairs"] == 150
    assert host[1]["chunks"] == 1 if chunk_bytes > 65281 else host[1]["chunks"] >= os.path.getsize(f["r1"]) // chunk_bytes
    _same(scan_pair_end_report(f["fa"], f["csvs"][3], f["z1"], f["z2"], chunk_bytes=chunk_bytes, inflate="device"), host)


def test_single_end_multi_csv_and_the_reference(gpu_device, files):
    from genefuserust_amd.multi_csv_scan import scan_multi_csv_report, scan_report
    from genefuserust_amd.scan import open_index, scan_pair_end_files, scan_single_end_report
    f = files
    c = 9000
    host = scan_single_end_report(f["fa"], f["csvs"][1], f["z1"], chunk_bytes=c, inflate="host")
    assert host[1]["fusions"] >= 1 and host[1]["chunks"] >= 3
    _same(scan_single_end_report(f["fa"], f["csvs"][1], f["z1"], chunk_bytes=c, inflate="device"), host)
    # two CSVs, one streamed pass
    lst = f["tmp"] / "two.txt"
    lst.write_text("%s\n%s\n" % (f["csvs"][0], f["csvs"][1]))
    h = scan_multi_csv_report(f["fa"], str(lst), f["z1"], f["z2"], chunk_bytes=c, inflate="host")
    d = scan_multi_csv_report(f["fa"], str(lst), f["z1"], f["z2"], chunk_bytes=c, inflate="device")
    assert [x[0] for x in d] == [x[0] for x in h] == f["csvs"][:2]
    for (_, d_res, d_cnt), (_, h_res, h_cnt) in zip(d, h):
        _same((d_res, d_cnt), (h_res, h_cnt))
        assert h_cnt["fusions"] >= 1
    # the reference, BGZF, cut on the device from inflated chunks: the same index
    for rc_ in (64, 4096, 1 << 20):
        with open_index(f["zfa"], f["csvs"][3], ref_chunk_bytes=rc_, inflate="host") as (hx, _), \
                open_index(f["zfa"], f["csvs"][3], ref_chunk_bytes=rc_, inflate="device") as (dx, _):
            assert list(dx.m_fusion_seq) == list(hx.m_fusion_seq) and len(hx.m_fusion_seq) >= 2
            assert dx.info() == hx.info()
    # both at once, through the mode switch; and the keyword reaches the list mode
    both = scan_report(f["zfa"], f["csvs"][3], f["z1"], f["z2"], chunk_bytes=c, ref_chunk_bytes=4096, inflate="device")
    _same(both, scan_report(f["zfa"], f["csvs"][3], f["z1"], f["z2"], chunk_bytes=c, ref_chunk_bytes=4096))
    d = scan_report(f["zfa"], str(lst), f["z1"], f["z2"], ref_chunk_bytes=4096, inflate="device")
    h = scan_report(f["zfa"], str(lst), f["z1"], f["z2"], ref_chunk_bytes=4096)
    assert [(x[0], _texts(x[1]), x[2]) for x in d] == [(x[0], _texts(x[1]), x[2]) for x in h]
    # matches and counters of the files route
    dm, dc = scan_pair_end_files(f["fa"], f["csvs"][0], f["z1"], f["z2"], chunk_bytes=c, inflate="device")
    hm, hc = scan_pair_end_files(f["fa"], f["csvs"][0], f["z1"], f["z2"], chunk_bytes=c)
    assert dc == hc and [(m.m_name, m.m_read) for m in dm] == [(m.m_name, m.m_read) for m in hm] and len(hm) >= 1


def test_auto_decides_per_file(gpu_device, files):
    from genefuserust_amd.scan import scan_pair_end_report
    f = files
    plain_gz = str(f["tmp"] / "R2_plain.fq.gz")
    with gzip.open(plain_gz, "wb") as out:
        out.write(open(f["r2"], "rb").read())
    c = 9000
    host = scan_pair_end_report(f["fa"], f["csvs"][3], f["z1"], plain_gz, chunk_bytes=c)
    _same(scan_pair_end_report(f["fa"], f["csvs"][3], f["z1"], plain_gz, chunk_bytes=c, inflate="auto"), host)
    _same(scan_pair_end_report(f["fa"], f["csvs"][3], f["z1"], f["r2"], chunk_bytes=c, inflate="auto"), host)
    _same(scan_pair_end_report(f["fa"], f["csvs"][3], f["r1"], f["z2"], chunk_bytes=c, inflate="device"), host)
    # strict: the plain gzip file is named
    with pytest.raises(ValueError) as e:
        scan_pair_end_report(f["fa"], f["csvs"][3], f["z1"], plain_gz, chunk_bytes=c, inflate="device")
    assert plain_gz in str(e.value)


def test_value_errors(gpu_device, files):
    from genefuserust_amd.multi_csv_scan import scan_multi_csv_report, scan_report
    from genefuserust_amd.scan import (open_index, scan_pair_end_files, scan_pair_end_report, scan_single_end_files,
                                       scan_single_end_report)
    f = files
    for mode in ("auto", "device"):     # neither file is streamed: the whole-file routes read text()
        for call in (lambda: scan_pair_end_report(f["fa"], f["csvs"][0], f["z1"], f["z2"], inflate=mode),
                     lambda: scan_pair_end_files(f["fa"], f["csvs"][0], f["z1"], f["z2"], inflate=mode),
                     lambda: scan_single_end_report(f["fa"], f["csvs"][0], f["z1"], inflate=mode),
                     lambda: scan_single_end_files(f["fa"], f["csvs"][0], f["z1"], inflate=mode),
                     lambda: scan_multi_csv_report(f["fa"], f["lst"], f["z1"], f["z2"], inflate=mode),
                     lambda: scan_report(f["fa"], f["csvs"][0], f["z1"], f["z2"], inflate=mode),
                     lambda: open_index(f["zfa"], f["csvs"][0], inflate=mode).__enter__()):
            with pytest.raises(ValueError, match="chunk_bytes"):
                call()
    with pytest.raises(ValueError, match="inflate"):
        scan_pair_end_report(f["fa"], f["csvs"][0], f["z1"], f["z2"], chunk_bytes=9000, inflate="gpu")
    # the refusal of chunk_bytes for a list of CSVs stays
    with pytest.raises(ValueError, match="chunk_bytes"):
        scan_report(f["fa"], f["lst"], f["z1"], f["z2"], chunk_bytes=9000, inflate="device")
    # a member that is not BGZF behind the first: the file, the offset, and the way out
    text = open(f["r1"], "rb").read()
    mixed = str(f["tmp"] / "mixed.fq.gz")
    first = bm.member(text[:4000])
    open(mixed, "wb").write(first + gzip.compress(text[4000:]))
    with pytest.raises(ValueError) as e:
        scan_single_end_report(f["fa"], f["csvs"][0], mixed, chunk_bytes=9000, inflate="device")
    assert mixed in str(e.value) and "offset %d" % len(first) in str(e.value) and 'inflate="host"' in str(e.value)
    assert scan_single_end_report(f["fa"], f["csvs"][0], mixed, chunk_bytes=9000)[1]["reads"] == 150


def test_a_bad_member_and_a_cut_file(gpu_device, files):
    from genefuserust_amd.scan import open_index, scan_pair_end_report, scan_single_end_report
    f = files
    text = open(f["r1"], "rb").read()
    members = [bm.member(text[k:k + 4000]) for k in range(0, len(text), 4000)]
    assert len(members) >= 5
    third = bytearray(members[2])
    third[-8] ^= 1                                  # its CRC-32
    bad = str(f["tmp"] / "bad_crc.fq.gz")
    open(bad, "wb").write(b"".join(members[:2]) + bytes(third) + b"".join(members[3:]) + bm.EOF_MARKER)
    offset = len(members[0]) + len(members[1])
    for c in (4096, 1 << 20):
        with pytest.raises(gzip.BadGzipFile) as e:
            scan_single_end_report(f["fa"], f["csvs"][0], bad, chunk_bytes=c, inflate="device")
        assert bad in str(e.value) and "offset %d" % offset in str(e.value) and "CRC" in str(e.value)
        with pytest.raises(gzip.BadGzipFile):
            scan_single_end_report(f["fa"], f["csvs"][0], bad, chunk_bytes=c, inflate="host")
    # as R2 of a pair: the error of the further side's thread reaches the consumer
    with pytest.raises(gzip.BadGzipFile):
        scan_pair_end_report(f["fa"], f["csvs"][0], f["z1"], bad, chunk_bytes=9000, inflate="device")
    whole = open(f["z1"], "rb").read()
    for cut in (len(whole) - 28 - 3, len(whole) // 2):
        short = str(f["tmp"] / ("cut_%d.fq.gz" % cut))
        open(short, "wb").write(whole[:cut])
        for mode in ("device", "host"):
            with pytest.raises(EOFError):
                scan_single_end_report(f["fa"], f["csvs"][0], short, chunk_bytes=9000, inflate=mode)
    zfa = open(f["zfa"], "rb").read()
    short = str(f["tmp"] / "cut.fa.gz")
    open(short, "wb").write(zfa[:len(zfa) // 2])
    with pytest.raises(EOFError):
        open_index(short, f["csvs"][0], ref_chunk_bytes=4096, inflate="device").__enter__()
    # the scans that follow are whole
    _same(scan_single_end_report(f["fa"], f["csvs"][0], f["z1"], chunk_bytes=9000, inflate="device"),
          scan_single_end_report(f["fa"], f["csvs"][0], f["z1"], chunk_bytes=9000))
