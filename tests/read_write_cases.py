"""The cases the FASTQ output is held to the model on (tests/read_write_model.py), on the host and on the device: name
lines around the piece's and the round's sizes, kept lengths around the piece's, pairs out of step, tags.  Seeded;
nothing here looks at the library's code."""
from tests import read_write_model as model
from tests.umi_cases import fastq_text, random_bases, random_quals

# the lengths records keep: around a piece of 16 bytes and two, a usual read and one more, one above GF_MAX_READ_LEN
KEPT = [0, 1, 15, 16, 17, 31, 32, 33, 150, 151, 5000]
KEPT_SMALL = [0, 1, 15, 16, 17, 31, 32, 33, 150, 151]
# the name lines' lengths: around a piece, and around a round of 16 pieces
NAME_LENGTHS = [2, 15, 16, 17, 255, 256, 257]
NAME_BYTES = b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789:_/#"
UMI_LENGTHS = [1, 8, 32]


def name_line(rng, length: int, kind: int) -> bytes:
    """A name line of ``length`` bytes.  ``kind`` % 4: no space or tab; a space somewhere; a tab somewhere; a '\\r' at
    the end (with a space in front of it when the line has room)."""
    body = bytearray(b"@" + bytes(NAME_BYTES[int(k)] for k in rng.integers(0, len(NAME_BYTES), length - 1)))
    kind %= 4
    if kind in (1, 2):
        body[int(rng.integers(1, length))] = ord(" ") if kind == 1 else ord("\t")
    elif kind == 3:
        body[length - 1] = ord("\r")
        if length > 4:
            body[int(rng.integers(1, length - 1))] = ord(" ")
    return bytes(body)


def build(rng, n: int, sides: int, source: int = model.NAME, length: int = 0, skip: int = 0, final_newline: bool = True,
          kept=KEPT):
    """``n`` records (pairs with ``sides`` 2) as a call sees them: per side the FASTQ text of the records as the
    sequencer wrote them, the records ahead of the UMI cut (the text's), and the records as the steps left them — the
    UMI and its spacer off the mates that carry one, then a prefix of ``kept`` lengths, the mates out of step so that
    every combination of an empty side and a kept one occurs."""
    K = len(kept)
    texts, finals, pre = [], [], []
    for s in range(sides):
        takes = source == model.PER_READ or source == (model.READ2 if s else model.READ1)
        c = length + skip if takes else 0
        names, originals, left = [], [], []
        for i in range(n):
            keep = kept[(i + 5 * s) % K] if s == 0 else kept[(i // K + 3 * i) % K]
            total = c + keep + (i + s) % 3
            b, q = random_bases(rng, total), random_quals(rng, total)
            names.append(name_line(rng, NAME_LENGTHS[(i + 3 * s) % len(NAME_LENGTHS)], i // len(NAME_LENGTHS) + s))
            originals.append((b, q))
            left.append((b[c:c + keep], q[c:c + keep]))
        texts.append(fastq_text(names, originals, final_newline=final_newline))
        finals.append(left)
        pre.append(originals)
    return texts, finals, pre
