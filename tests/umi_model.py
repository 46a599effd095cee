"""The predicate of include/gf_umi.h in plain Python: the inline cut, the codes, the name parser, the key mixing and
the totals.  What libgfumi.so is held to, on the host (tests/test_umi_core.py) and on the device
(tests/test_umi_gpu.py).  ``H``, ``mix`` and ``key`` are those of the duplicate removal's model.  Nothing here looks at
the library's code."""
from collections import namedtuple

from tests.dedup_model import H, key, mix  # noqa: F401  (key: re-exported for the tests)

NAME, READ1, READ2, PER_READ = 0, 1, 2, 3
SOURCES = {"name": NAME, "read1": READ1, "read2": READ2, "per_read": PER_READ}
MAX_LEN, MAX_SKIP, MAX_FIELD, TOTALS = 32, 32, 64, 7
FIELD_BYTES = frozenset(b"ACGTNacgtn+_")


def settings_ok(source, length, skip) -> bool:
    if source == NAME:
        return length == 0 and skip == 0
    return source in (READ1, READ2, PER_READ) and 1 <= length <= MAX_LEN and 0 <= skip <= MAX_SKIP


def code(u: bytes) -> int:
    """U of one UMI."""
    return H(u) or 1


def code_pair(u1: bytes, u2: bytes) -> int:
    return mix(H(u1) + mix(H(u2) + 1)) or 1


def mix_key(K: int, U: int) -> int:
    """K' of a record with key K and code U."""
    if K == 0 or U == 0:
        return K
    return mix(K + mix(U + 2)) or 1


def has_n(u: bytes) -> bool:
    return b"N" in u or b"n" in u


Cut = namedtuple("Cut", "records codes totals")


def cut(source: int, length: int, skip: int, records) -> Cut:
    """The inline sources.  ``records``: a list of reads, each (bases, quals), or of pairs of them.  Gives the records
    as they leave (same shape), the codes and the seven totals."""
    assert source != NAME and settings_ok(source, length, skip)
    c = length + skip
    out, codes, totals = [], [], [0] * TOTALS
    for rec in records:
        pair = isinstance(rec[0], tuple)
        sides = list(rec) if pair else [rec]
        if not pair:
            assert source != READ2
        takes = [source in (READ1, PER_READ), source in (READ2, PER_READ)][:len(sides)]
        totals[0] += 1
        if any(t and len(s[0]) < c for t, s in zip(takes, sides)):
            totals[5] += 1
            totals[6] += sum(len(s[0]) for s in sides)
            new = [(b"", b"") for _ in sides]
            codes.append(0)
        else:
            umis = [s[0][:length] for t, s in zip(takes, sides) if t]
            new = [(s[0][c:], s[1][c:]) if t else s for t, s in zip(takes, sides)]
            U = code_pair(*umis) if len(umis) == 2 else code(umis[0])
            codes.append(U)
            totals[1] += 1
            totals[3] += any(has_n(u) for u in umis)
            totals[4] += c * len(umis)
        out.append(tuple(new) if pair else new[0])
    return Cut(out, codes, totals)


def name_line(text: bytes, i: int):
    """The name line of record ``i`` as gf_hit_names.h defines it, None when the text has no such line."""
    nl = [k for k, ch in enumerate(text) if ch == 10]
    line = 4 * i
    if line > len(nl):
        return None
    s = 0 if line == 0 else nl[line - 1] + 1
    e = nl[line] if line < len(nl) else len(text)
    return text[s:e]


def name_field(line: bytes):
    """The UMI field of a name line, None when it has none."""
    if line.endswith(b"\r"):
        line = line[:-1]
    end = min([k for k in (line.find(b" "), line.find(b"\t")) if k >= 0] + [len(line)])
    token = line[:end]
    colon = token.rfind(b":")
    if colon < 0:
        return None
    field = token[colon + 1:]
    if not 1 <= len(field) <= MAX_FIELD or not set(field) <= FIELD_BYTES:
        return None
    return field


def names(text: bytes, n: int):
    """The name source over the first ``n`` records of ``text``: (codes, totals)."""
    codes, totals = [], [0] * TOTALS
    for i in range(n):
        line = name_line(text, i)
        field = None if line is None else name_field(line)
        totals[0] += 1
        if field is None:
            codes.append(0)
            totals[2] += 1
        else:
            codes.append(code(field))
            totals[1] += 1
            totals[3] += has_n(field)
    return codes, totals


def dedup_keys(records, codes):
    """The keys a deduplication with codes offers: K' of every read or pair."""
    return [mix_key(key(*[s[0] for s in r]) if isinstance(r[0], tuple) else key(r[0]), U)
            for r, U in zip(records, codes)]
