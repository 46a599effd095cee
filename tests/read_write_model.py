"""The predicate of include/gf_read_write.h in plain Python: which records are written, their four lines, the tag and the
totals — over records as the other models leave them (tests/umi_model.py, tests/adapter_trim_model.py,
tests/read_filter_model.py, tests/dedup_model.py).  What libgfwrite.so is held to, on the host
(tests/test_read_write_core.py) and on the device (tests/test_read_write_gpu.py).  Nothing here looks at the library's
code."""
from collections import namedtuple

from tests import umi_model
from tests.umi_model import NAME, PER_READ, READ1, READ2, SOURCES  # noqa: F401  (re-exported for the tests)

TAG_MAX, TOTALS, MAX_LEN = 1 + 32 + 1 + 32, 5, 32
WIDE, BYTES = 0, 1


def settings_ok(source, length, gather) -> bool:
    if gather not in (WIDE, BYTES):
        return False
    if source == NAME:
        return length == 0
    return source in (READ1, READ2, PER_READ) and 1 <= length <= MAX_LEN


def capacity(text_bytes: int, n: int) -> int:
    return text_bytes + 1 + n * TAG_MAX


def name_line(text: bytes, i: int) -> bytes:
    """The name line of record ``i``; empty when the text has no such line."""
    line = umi_model.name_line(text, i)
    return b"" if line is None else line


def name_lines(text: bytes, n: int):
    """``name_line`` of the records 0 .. n - 1, with the text's newlines looked up once."""
    nl, at = [], text.find(b"\n")
    while at >= 0:
        nl.append(at)
        at = text.find(b"\n", at + 1)
    out = []
    for i in range(n):
        line = 4 * i
        if line > len(nl):
            out.append(b"")
        else:
            out.append(text[0 if line == 0 else nl[line - 1] + 1:nl[line] if line < len(nl) else len(text)])
    return out


def token_end(line: bytes) -> int:
    """The length of the line's first token: up to the first space or tab, or the whole line."""
    return min([k for k in (line.find(b" "), line.find(b"\t")) if k >= 0] + [len(line)])


def tag(source: int, length: int, pre) -> bytes:
    """The tag of a record whose pre-cut bases are ``pre`` (one per side); empty for ``NAME``."""
    if source == NAME:
        return b""
    if source == PER_READ and len(pre) == 2:
        return b":" + pre[0][:length] + b"_" + pre[1][:length]
    return b":" + pre[1 if source == READ2 and len(pre) == 2 else 0][:length]


def tagged_name(line: bytes, t: bytes) -> bytes:
    end = token_end(line) if t else len(line)
    return line[:end] + t + line[end:]


def record_text(line: bytes, t: bytes, bases: bytes, quals: bytes) -> bytes:
    return tagged_name(line, t) + b"\n" + bases + b"\n+\n" + quals + b"\n"


Formatted = namedtuple("Formatted", "texts offsets totals written")


def format_reads(texts, finals, source: int = NAME, length: int = 0, pre=None) -> Formatted:
    """One ``gf_rw_format_device`` call.  ``texts``: per side the FASTQ text the records were cut from; ``finals``: per
    side the records (bases, quals) as the last step left them; ``pre``: per side the records ahead of the UMI cut
    (with a tag).  Gives per side the output text and its n + 1 offsets, the five totals and the written flags."""
    sides, n = len(texts), len(finals[0])
    assert sides in (1, 2) and all(len(f) == n for f in finals) and settings_ok(source, length, WIDE)
    assert not (sides == 1 and source == READ2)
    out, offsets, totals, flags = [bytearray() for _ in texts], [[0] for _ in texts], [0] * TOTALS, []
    names = [name_lines(text, n) for text in texts]
    for i in range(n):
        written = all(len(f[i][0]) > 0 for f in finals)
        flags.append(written)
        if written:
            t = tag(source, length, [p[i][0] for p in pre]) if source != NAME else b""
            for s in range(sides):
                out[s] += record_text(names[s][i], t, finals[s][i][0], finals[s][i][1])
            totals[0] += 1
            totals[1] += sum(len(f[i][0]) for f in finals)
        else:
            totals[4] += 1
        for s in range(sides):
            offsets[s].append(len(out[s]))
    for s in range(sides):
        totals[2 + s] = len(out[s])
    return Formatted([bytes(o) for o in out], offsets, totals, flags)


def counters(totals) -> dict:
    return {"written_records": totals[0], "written_bases": totals[1], "written_bytes": totals[2] + totals[3]}
