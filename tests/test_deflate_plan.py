"""gf_df_plan (genefuserust_amd/scan_csrc/gf_df_core.h) on histograms given to it directly, through the ``plan`` job of
the stand-alone host program (tests/cpp/test_deflate_core.cpp, g++ under AddressSanitizer and
UndefinedBehaviorSanitizer): the three codes of a member — literal/length and distance within 15 bits, the code-length
code within 7 — against tests/huffman_model.py, which shares nothing with the construction under test.  The texts of
tests/deflate_cases.py rarely push a code against its limit; the histograms here do so hundreds of times each, and the
test counts that on the model alone before it looks at the program's answers.

What the construction promises and the test holds it to: a complete code within the limit, never a longer code for a
strictly more frequent symbol, the optimum exactly where the limit does not bind.  Where it binds the code is a
heuristic (counts per length pushed down, the longest codes to the rarest symbols): its cost over the optimum under
the limit is printed, and DESIGN.md records the largest ratio; it is not asserted."""
import collections

import numpy as np
import pytest

from tests import bgzf_members as bm
from tests import huffman_model as hm
from tests.test_deflate_core import program, run   # noqa: F401  (the same program, the same flags)

NLIT, NDIST, NCL, EOB = 286, 30, 19, 256
MAX_MATCHES = 13056          # 65280 / 5: a match covers at least gf_df_min_len(1) = 5 bytes
TEXT = 65280
LIMITS = {"literal": 15, "distance": 15, "code_length": 7}


def fib(n):
    out, a, b = [], 1, 2
    while len(out) < n:
        out.append(a)
        a, b = b, a + b
    return out


def doubling(n):
    return [1 << k for k in range(n)]


def tail_counts(n, series, budget, most):
    """``n`` counts: the first min(n, most) values of ``series`` (cut so that they sum to at most ``budget``), the
    other symbols equal and as large as the budget allows, at least 1."""
    tail = series(min(n, most))
    while sum(tail) > budget:
        tail.pop()
    rest = n - len(tail)
    return tail + [max(1, min(tail[-1], (budget - sum(tail)) // rest))] * rest if rest else tail


def spread(counts, nsym, rng):
    """The counts on randomly chosen symbols of an alphabet of ``nsym``."""
    out = [0] * nsym
    for c, s in zip(counts, rng.permutation(nsym)[:len(counts)]):
        out[int(s)] = int(c)
    return out


def joint(lit, dist):
    lit, dist = list(lit) + [0] * (NLIT - len(lit)), list(dist) + [0] * (NDIST - len(dist))
    assert len(lit) == NLIT and len(dist) == NDIST
    return lit + dist


def dyadic_for_the_code_length_code():
    """A literal histogram whose optimal code has 1, 1, 2, 3, 5, 8, 13, 21, 34, 55 and 89 symbols of eleven different
    lengths — counts 2^(15 - length), so that the lengths are forced — and 85 unused literals: the histogram of the
    lengths themselves is a Fibonacci one, and the code-length code wants 8 bits and more."""
    per_length = _kraft_assignment(fib(2)[:1] + fib(10), list(range(4, 16)))
    lit, s = [0] * NLIT, 0
    for length, n in sorted(per_length.items()):
        for _ in range(n):
            if s == EOB:
                s += 1
            lit[s] = 1 << (15 - length)
            s += 1
    # the end-of-block symbol is one of the rarest
    last = max(k for k in range(EOB) if lit[k])
    lit[EOB], lit[last] = lit[last], 0
    return lit


def _kraft_assignment(numbers, lengths):
    """{length: how many symbols}: ``numbers`` put on different ``lengths`` so that the Kraft sum is exactly 1."""
    unit = 1 << max(lengths)

    def place(k, left, free):
        if k == len(numbers):
            return {} if left == 0 else None
        for l in free:
            w = numbers[k] * (unit >> l)
            if w <= left:
                got = place(k + 1, left - w, [x for x in free if x != l])
                if got is not None:
                    got[l] = numbers[k]
                    return got
        return None
    got = place(0, unit, lengths)
    assert got is not None
    return got


def histograms():
    """[(name, 316 counts)]"""
    rng = np.random.default_rng(1951)
    out = []
    # the crafted ones: every limit binds
    lit = [0] * NLIT
    for k, c in enumerate([1] + fib(24)):
        lit[EOB - k] = c                         # the end-of-block symbol is the rarest
    out.append(("fibonacci_24_literals_19_distances", joint(lit, spread(fib(19), NDIST, rng))))
    out.append(("dyadic_lengths_in_fibonacci_numbers", joint(dyadic_for_the_code_length_code(), [])))
    # Fibonacci and doubling tails on 2 .. 286 literal/length symbols and on 1 .. 30 distance symbols
    for kind, series, most_lit, most_dist in (("fibonacci", fib, 22, 19), ("doubling", doubling, 15, 13)):
        for n in range(2, NLIT + 1):
            m = 1 + (n - 2) % NDIST
            lit = spread(tail_counts(n - 1, series, TEXT, most_lit), NLIT - 1, rng)
            lit = lit[:EOB] + [1] + lit[EOB:]    # a member has exactly one end-of-block symbol
            dist = spread(tail_counts(m, series, MAX_MATCHES, most_dist), NDIST, rng)
            assert sum(dist) <= MAX_MATCHES
            out.append(("%s_tail_%d_literals_%d_distances" % (kind, n, m), joint(lit, dist)))
    for c in (1, 7, 228):
        out.append(("all_equal_%d" % c, joint([c] * NLIT, [c] * NDIST)))
    out.append(("two_symbols", joint(spread([5], EOB, rng) + [1], spread([3, 2], NDIST, rng))))
    out.append(("two_equal_symbols", joint(spread([1], EOB, rng) + [1], spread([1, 1], NDIST, rng))))
    out.append(("end_of_block_alone", joint([0] * EOB + [1], [])))
    for s in range(NDIST):
        lit = spread(rng.integers(1, 400, 40), EOB, rng) + [1] + [0] * 29
        lit[257 + s % 29] = 9
        dist = [0] * NDIST
        dist[s] = 9
        out.append(("one_distance_symbol_%d" % s, joint(lit, dist)))
    out.append(("no_distance_symbol", joint(spread(rng.integers(1, 400, 40), EOB, rng) + [1], [])))
    # heavy tails at random, totals a member can have: geometric literals with distances in a chain like Fibonacci's (deep literal and distance codes), power laws (the
    # numbers of symbols per length grow like Fibonacci's: deep code-length codes), log-normal
    for k in range(2400):
        def heavy(n, total, kind):
            ranks = np.arange(1, n + 1, dtype=np.float64)
            if kind == 0:
                w = rng.uniform(0.35, 0.75) ** ranks
            elif kind == 1:
                w = ranks ** -rng.uniform(1.1, 1.9)
            else:
                w = np.exp(rng.normal(0, rng.uniform(1.5, 4.0), n))
            w *= np.exp(rng.normal(0, 0.15, n))
            c = np.maximum(1, np.floor(w / w.sum() * total * rng.uniform(0.3, 0.95))).astype(np.int64)
            return [int(x) for x in c]
        kind = k % 3
        n_lit = int(rng.integers(2, NLIT)) if kind != 1 else int(rng.integers(150, NLIT))
        lit = spread(heavy(n_lit, TEXT, kind), NLIT - 1, rng)
        lit = lit[:EOB] + [1] + lit[EOB:]
        if kind == 0:
            # 13056 matches pass 15 bits only where the counts grow hardly faster than Fibonacci's numbers (19 of those
            # sum to 10945): each count the sum of the two before it and a random slack, on 14 .. 19 symbols
            c = [1, int(rng.integers(1, 3))]
            for _ in range(int(rng.integers(12, 18))):
                c.append(c[-1] + c[-2] + int(rng.integers(0, 1 + c[-1] // 8)))
            while sum(c) > MAX_MATCHES:
                c.pop()
        else:
            c = heavy(int(rng.integers(0, NDIST + 1)), MAX_MATCHES, kind)
        n_dist, dist = len(c), spread(c, NDIST, rng)
        if n_dist == 0:
            lit[257:] = [0] * 29                 # no distance, no length
        assert sum(lit) <= TEXT + 1 and sum(dist) <= MAX_MATCHES
        out.append(("random_%d" % k, joint(lit, dist)))
    return out


def model(freq):
    """What the reference alone says of a histogram: per code (unrestricted optimum, optimum within the limit), and the
    code-length histogram of the reference's own literal/length and distance codes."""
    lit, dist = freq[:NLIT], freq[NLIT:]
    out, lens = {}, {}
    for name, f in (("literal", lit), ("distance", dist)):
        out[name] = (hm.huffman_cost(f), hm.limited_cost(f, 15))
        lens[name] = hm.huffman_lengths(f)
        if max(lens[name], default=0) > 15:
            lens[name] = hm.limited_lengths(f, 15)
    hlit = max([257] + [s + 1 for s in range(257, NLIT) if lens["literal"][s]])
    hdist = max([1] + [s + 1 for s in range(1, NDIST) if lens["distance"][s]])
    cl = [0] * NCL
    for l in lens["literal"][:hlit] + lens["distance"][:hdist]:
        cl[l] += 1
    out["code_length"] = (hm.huffman_cost(cl), hm.limited_cost(cl, 7))
    return out


@pytest.fixture(scope="module")
def plans(program, tmp_path_factory):   # noqa: F811
    """[(name, counts, lens[316], cl_lens[19], cl_freq[19], hlit, hdist, bits)]: every histogram through the program."""
    tmp = tmp_path_factory.mktemp("deflate_plans")
    hs = histograms()
    for k, (_, freq) in enumerate(hs):
        (tmp / ("h%d" % k)).write_text(" ".join(str(c) for c in freq) + "\n")
    answers = run(program, tmp, ["plan %s" % (tmp / ("h%d" % k)) for k in range(len(hs))])
    out = []
    for (name, freq), a in zip(hs, answers):
        a = [int(x) for x in a]
        assert len(a) == 316 + 19 + 19 + 3, name
        out.append((name, freq, a[:316], a[316:335], a[335:354], a[354], a[355], a[356]))
    return out


def test_the_histograms_bind_every_limit_on_the_reference_alone():
    hs = histograms()
    assert sum(1 for name, _ in hs if name.startswith("random_")) >= 2000
    binding = collections.Counter()
    for name, freq in hs:
        for code, (free, limited) in model(freq).items():
            assert limited >= free
            binding[code] += limited > free
    print("histograms", len(hs), "binding", dict(binding))
    for code in LIMITS:
        assert binding[code] >= 100, (code, binding[code])
    # the crafted ones: unrestricted depths 24 and 18, and 8 for the code-length code
    crafted = dict(hs[:2])
    f = crafted["fibonacci_24_literals_19_distances"]
    assert hm.huffman_depth(f[:NLIT]) == 24 and hm.huffman_depth(f[NLIT:]) == 18
    m = model(crafted["dyadic_lengths_in_fibonacci_numbers"])
    assert m["code_length"][1] > m["code_length"][0]


def check_code(name, code, freq, lens, limit):
    """The properties of one code; returns (cost, unrestricted optimum, optimum within the limit)."""
    used = [s for s, f in enumerate(freq) if f]
    for s, (f, l) in enumerate(zip(freq, lens)):
        assert (l == 0) if f == 0 else (1 <= l <= limit), (name, code, s, f, l)
    if len(used) == 0:
        assert code == "distance"
    elif len(used) == 1:
        assert lens[used[0]] == 1
    else:
        assert hm.kraft(lens, limit) == 1 << limit, (name, code, "Kraft", hm.kraft(lens, limit))
    longest = 0                              # among the strictly more frequent symbols
    by_count = collections.defaultdict(list)
    for s in used:
        by_count[freq[s]].append(lens[s])
    for f in sorted(by_count, reverse=True):
        assert min(by_count[f]) >= longest, (name, code, "a more frequent symbol with a longer code", f)
        longest = max(longest, max(by_count[f]))
    cost, free, limited = hm.cost(freq, lens), hm.huffman_cost(freq), hm.limited_cost(freq, limit)
    assert cost >= limited >= free, (name, code, cost, limited, free)
    if limited == free:
        assert cost == free, (name, code, "the limit does not bind", cost, free)
    return cost, free, limited


def test_every_plan_is_complete_monotone_and_optimal_where_the_limit_does_not_bind(plans):
    worst = {code: (1.0, None) for code in LIMITS}
    bound = collections.Counter()
    for name, freq, lens, cl_lens, cl_freq, hlit, hdist, bits in plans:
        lit, dist = freq[:NLIT], freq[NLIT:]
        assert hlit == max([257] + [s + 1 for s in range(257, NLIT) if lit[s]]), name
        assert hdist == max([1] + [s + 1 for s in range(1, NDIST) if dist[s]]), name
        # the code-length histogram is that of the lengths the header carries
        want = [0] * NCL
        for l in lens[:hlit] + lens[NLIT:NLIT + hdist]:
            want[l] += 1
        if sum(1 for c in want if c) == 1:   # a code of one symbol is incomplete: a second symbol joins it
            want[1 if want[0] else 0] = 1
        assert cl_freq == want, name
        results = {"literal": check_code(name, "literal", lit, lens[:NLIT], 15),
                   "distance": check_code(name, "distance", dist, lens[NLIT:], 15),
                   "code_length": check_code(name, "code_length", cl_freq, cl_lens, 7)}
        for code, (cost, free, limited) in results.items():
            if limited > free:
                bound[code] += 1
                ratio = cost / limited
                print("%s %s cost %d optimum within the limit %d ratio %.5f" % (name, code, cost, limited, ratio))
                if ratio > worst[code][0]:
                    worst[code] = (ratio, name)
        header = 3 + 5 + 5 + 4 + 3 * NCL + sum(cl_lens[l] for l in lens[:hlit] + lens[NLIT:NLIT + hdist])
        body = sum(f * (l + (bm.LEN_EXTRA[s - 257] if s > 256 else 0)) for s, (f, l) in enumerate(zip(lit, lens[:NLIT])))
        body += sum(f * (l + bm.DIST_EXTRA[s]) for s, (f, l) in enumerate(zip(dist, lens[NLIT:])))
        assert bits == header + body, name
    print("limits bound on the program's own histograms:", dict(bound))
    print("largest cost over the optimum within the limit:", worst)
    # (the code-length histogram is the program's own here; on the reference's it is counted in the test above)
    assert bound["literal"] >= 100 and bound["distance"] >= 100 and bound["code_length"] >= 100
