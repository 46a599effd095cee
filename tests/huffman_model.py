"""Prefix codes in plain Python, for holding gf_df_code_lengths (genefuserust_amd/scan_csrc/gf_df_core.h) to what a code
can cost at best: the unrestricted optimum (Huffman, by heap), the optimum under a length limit (package-merge: Larmore
and Hirschberg 1990) and the Kraft sum.  Nothing here is shared with the code under test: no in-place construction, no
counts per length, no push-down."""
import heapq


def _used(freq):
    return [(int(f), s) for s, f in enumerate(freq) if f]


def huffman_lengths(freq):
    """Code lengths of an optimal prefix code, 0 for unused symbols.  Among equal weights the shallower subtree is
    merged first, which gives the optimal code of the least depth.  One used symbol: length 1."""
    lens = [0] * len(freq)
    used = _used(freq)
    if len(used) == 1:
        lens[used[0][1]] = 1
    if len(used) < 2:
        return lens
    heap = [(f, 0, k, (s,)) for k, (f, s) in enumerate(used)]      # weight, height, tie-break, leaves
    heapq.heapify(heap)
    k = len(heap)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        for s in a[3] + b[3]:
            lens[s] += 1
        heapq.heappush(heap, (a[0] + b[0], max(a[1], b[1]) + 1, k, a[3] + b[3]))
        k += 1
    return lens


def huffman_cost(freq) -> int:
    """sum(count * length) of an optimal prefix code: the sum of the merged weights."""
    heap = [f for f, _ in _used(freq)]
    if len(heap) == 1:
        return heap[0]
    heapq.heapify(heap)
    cost = 0
    while len(heap) > 1:
        w = heapq.heappop(heap) + heapq.heappop(heap)
        cost += w
        heapq.heappush(heap, w)
    return cost


def huffman_depth(freq) -> int:
    return max(huffman_lengths(freq), default=0)


def limited_lengths(freq, limit: int):
    """Code lengths of an optimal prefix code whose lengths are at most ``limit``, by package-merge: ``limit`` lists of
    the leaves merged with the pairs of the list before; the first 2n - 2 items of the last list say how often each
    leaf is taken, which is its length."""
    lens = [0] * len(freq)
    used = sorted(_used(freq))
    n = len(used)
    if n == 1:
        lens[used[0][1]] = 1
    if n < 2:
        return lens
    assert (1 << limit) >= n, "no code of %d symbols within %d bits" % (n, limit)
    leaves = [(f, k, None, None) for k, (f, _) in enumerate(used)]        # weight, order, left, right
    items = list(leaves)
    for _ in range(limit - 1):
        packages = [(items[k][0] + items[k + 1][0], n + k, items[k], items[k + 1]) for k in range(0, len(items) - 1, 2)]
        items = sorted(leaves + packages, key=lambda it: (it[0], it[1]))
    stack = items[:2 * n - 2]
    while stack:
        it = stack.pop()
        if it[2] is None:
            lens[used[it[1]][1]] += 1
        else:
            stack += [it[2], it[3]]
    return lens


def cost(freq, lens) -> int:
    return sum(int(f) * l for f, l in zip(freq, lens))


def limited_cost(freq, limit: int) -> int:
    """The least sum(count * length) of a prefix code within ``limit`` bits.  Package-merge runs only where the
    shallowest Huffman code is deeper than the limit: else that code is the optimum under the limit too."""
    lens = huffman_lengths(freq)
    if max(lens, default=0) <= limit:
        return cost(freq, lens)
    return cost(freq, limited_lengths(freq, limit))


def kraft(lens, limit: int) -> int:
    """The Kraft sum of the lengths in use, in units of 2^-limit: a complete code gives 1 << limit."""
    return sum(1 << (limit - l) for l in lens if l)
