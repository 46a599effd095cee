"""The cases the UMI calls are held to the model on (tests/umi_model.py), on the host and on the device: name lines,
records around the UMI's length, FASTQ texts.  Seeded; nothing here looks at the library's code."""
import numpy as np

GRID = [(length, skip) for length in (1, 8, 15, 16, 17, 32) for skip in (0, 1, 32)]
JUNK = [0x00, 0xFF, ord("G"), ord("N"), ord(":"), ord(" ")]
ALPHABET = b"ACGTACGTACGTNacgtn"

FIELD_64 = (b"ACGTNacgtn+_" * 6)[:64]

# name lines (without '@' meaning anything: the parser takes the line as it is), each with whether it holds a UMI
NAME_CASES = [
    (b"@M01:23:FC:1:1101:15589:1332:ACGTNN 1:N:0:ATCACG", True),      # Illumina, the UMI behind the coordinates
    (b"@M01:23:FC:1:1101:15589:1333:ACGT+TTGA 1:N:0:ATCACG", True),   # dual
    (b"@M01:23:FC:1:1101:15589:1334:ACGT_TTGA 1:N:0:ATCACG", True),   # '_' between the halves
    (b"@M01:23:FC:1:1101:15589:1335:acgt+ttga 1:N:0:ATCACG", True),   # lower case: the same code as upper
    (b"@M01:23:FC:1:1101:15589:1336:ACGTACGT\t1:N:0:ATCACG", True),   # a tab ends the token
    (b"@read_without_a_colon ACGT:ACGT", False),                      # no ':' in the token
    (b"@M01:23:FC:1:1101:15589:1337: 1:N:0:ATCACG", False),           # a trailing ':'
    (b"@M01:23:FC:1:1101:15589:1338:", False),                        # ... at the line's end
    (b"@x:" + FIELD_64 + b" 1:N:0:A", True),                          # 64 bytes: taken
    (b"@x:" + FIELD_64 + b"A 1:N:0:A", False),                        # 65 bytes: refused
    (b"@M01:23:FC:1:1101:15589:1339:ACGTXCGT 1:N:0:ATCACG", False),   # one invalid byte
    (b"@M01:23:FC:1:1101:15589:1340:ACGT-TTGA", False),
    (b"@M01:23:FC:1:1101:15589:1341:ACGTACGT", True),                 # the token ends with the line
    (b"@M01:23:FC:1:1101:15589:1342:ACGTACGT\r", True),               # \r\n lines
    (b"@M01:23:FC:1:1101:15589:1343:ACGT \r", True),
    (b"@M01:23:FC:1:1101:15589:1344:\r", False),
    (b"@:A", True),
    (b":T", True),
    (b":", False),
    (b"", False),
    (b"\r", False),
    (b" :ACGT", False),                                               # an empty token
    (b"@" + b"x" * 300 + b":ACGTTGCA 1:N:0:A", True),                 # the colon in a later round of chunks
    (b"@a:" + b"C" * 20 + b" " + b"y" * 300 + b":ACGT", True),        # a long comment behind the token
    (b"@" + b"q:" * 140 + b"GATTACA", True),                          # colons in every chunk, the token 288 bytes
    (b"@M01:7:ACGT\x7fTTGA", False),                                  # DEL folds to '_' and is none
    (b"@M01:7:ACGT\x0bTTGA", False),                                  # VT is what '+' folds to
]


def random_bases(rng, n: int) -> bytes:
    return bytes(ALPHABET[int(k)] for k in rng.integers(0, len(ALPHABET), n))


def random_quals(rng, n: int) -> bytes:
    return bytes(int(k) for k in rng.integers(33, 74, n))


def record(rng, n: int):
    return random_bases(rng, n), random_quals(rng, n)


def lengths_around(c: int):
    """The record lengths of the GPU tests for a UMI of c bytes with its spacer."""
    return sorted({0, max(c - 1, 0), c, c + 1, 15, 16, 17, 150, 151, 5000})


def records_for(rng, n: int, c: int, pairs: bool):
    """``n`` reads or pairs whose lengths walk through ``lengths_around(c)``, the mates out of step, so that every
    combination of a short side and a long one occurs."""
    L = lengths_around(c)
    out = []
    for i in range(n):
        a = record(rng, L[i % len(L)])
        out.append((a, record(rng, L[(i // len(L) + 3 * i) % len(L)])) if pairs else a)
    return out


def fastq_text(names, records, crlf: bool = False, final_newline: bool = True) -> bytes:
    """A FASTQ text of the reads ``records`` ((bases, quals) each) under ``names`` (name lines without the newline)."""
    nl = b"\r\n" if crlf else b"\n"
    text = b"".join(n + nl + b + nl + b"+" + nl + q + nl for n, (b, q) in zip(names, records))
    return text if final_newline or not text else text[:-len(nl)]
