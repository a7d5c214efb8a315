"""A catalogue of wrong suffix arrays for the SA verifier, checked here on the CPU.

sas_verify / SAS_BUILD_VERIFY (k_verify_adj in csrc/build_lcp.hip) compare the suffixes of adjacent
ranks 32 chars at a time, mask the last block, and let the lengths decide when the compare runs off
the shorter suffix.  A wrong array tests one of those edges only if no other pair gives it away, so
the catalogue is built from adjacent swaps: in a true SA the suffixes strictly increase, and swapping
ranks r - 1 and r leaves SA[r - 2] < SA[r] and SA[r - 1] < SA[r + 1], hence exactly the pair at r out
of order.  Its lcp says which block of the compare has to notice, and whether a char or the lengths
decide.

This file holds the texts, corruptions() and the pickers (shared with tests/test_gpu_verify.py) and
tests the catalogue itself: the oracle's check_sa gives the expected verdict of every entry that a
u32 array can hold, a brute-force compare of the suffix bytes confirms the exactly-one-pair claim,
and every shape the GPU tests rely on is asserted to be present, from kasai_lcp."""
import functools

import numpy as np

from oracle import pyoracle as O

# lcps of the char-decided swaps: each side of the 32-char block edges, and a long one
DEPTHS = (0, 1, 31, 32, 33, 63, 64, 65, 95, 96, 97, 200)
BLOCK_DEPTHS = DEPTHS[2:]
# lcps of the swaps that only the lengths decide (70: the catalogue text's ending; 299: the zeros')
LEN_LCPS = (1, 32, 33, 64, 65, 70, 299)
CATALOGUE_LEN_LCPS = LEN_LCPS[:6]
ZEROS_LEN_LCPS = (1, 32, 33, 64, 65, 299)
ZEROS_N = 300


def catalogue_text():
    """For each depth d a random d-char block, [1] and 9 random chars, then the block again, [2] and
    9 random chars: two suffixes that differ first at char d (and their tails at every smaller
    depth).  Then a 70-char block, 13 random chars and the block again: each of the last 70
    suffixes is a proper prefix of an earlier one."""
    rng = np.random.default_rng(5)
    parts = []
    for d in BLOCK_DEPTHS:
        blk = rng.integers(0, 4, d, dtype=np.uint8)
        parts += [blk, [1], rng.integers(0, 4, 9, dtype=np.uint8), blk, [2], rng.integers(0, 4, 9, dtype=np.uint8)]
    blk = rng.integers(0, 4, 70, dtype=np.uint8)
    parts += [blk, rng.integers(0, 4, 13, dtype=np.uint8), blk]
    t = np.concatenate([np.asarray(p, np.uint8) for p in parts])
    t.setflags(write=False)
    return t


def zeros_text():
    """Its SA is n - 1, .., 0: the suffix of rank r has r + 1 chars, lcp[r] = r, and the lengths
    alone decide every pair."""
    t = np.zeros(ZEROS_N, np.uint8)
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def case(name):
    """(text, true SA as u32, lcp) of "catalogue" or "zeros", computed once and read-only."""
    t = {"catalogue": catalogue_text, "zeros": zeros_text}[name]()
    sa = O.build_sa(t)
    lcp = O.kasai_lcp(t, sa)
    for a in (sa, lcp):
        a.setflags(write=False)
    return t, sa, lcp


def pair_kinds(t, sa, lcp):
    """Per rank r >= 1 how the pair (r - 1, r) is decided: (by_char, by_length) boolean arrays.
    by_length: the shorter suffix is a prefix of the other, lcp == n - max(SA[r - 1], SA[r])."""
    n = len(t)
    s = sa.astype(np.int64)
    short = np.zeros(n, np.int64)
    short[1:] = n - np.maximum(s[:-1], s[1:])
    by_len = lcp.astype(np.int64) == short
    by_len[0] = False
    by_char = ~by_len
    by_char[0] = False
    return by_char, by_len


def swapped(sa, i, j, dtype):
    a = sa.astype(dtype)
    a[i], a[j] = a[j], a[i]
    return a


def corruptions(t, sa, width=4):
    """[(name, kind, array)]: kind "order" = every entry in range (swaps, one duplicate), "range" =
    one entry >= n.  width: the caller's entry bytes; 4 gives u32 arrays, 5 and 8 give u64 arrays
    (5: to be packed by pack40) with the values that only those widths hold.  Shapes that the text
    does not have (a depth, a length-decided lcp, a rank) are left out: the tests below say which
    text must hold which."""
    n = len(t)
    dtype = np.uint32 if width == 4 else np.uint64
    lcp = O.kasai_lcp(t, sa)
    by_char, by_len = pair_kinds(t, sa, lcp)
    out = []
    for d in DEPTHS:
        r = np.flatnonzero(by_char & (lcp == d))
        if len(r):
            out.append((f"char_lcp{d}", "order", swapped(sa, r[0] - 1, r[0], dtype)))
    for d in LEN_LCPS:
        r = np.flatnonzero(by_len & (lcp == d))
        if len(r):
            out.append((f"len_lcp{d}", "order", swapped(sa, r[0] - 1, r[0], dtype)))
    out.append(("first_pair", "order", swapped(sa, 0, 1, dtype)))
    out.append(("last_pair", "order", swapped(sa, n - 2, n - 1, dtype)))
    if n > 256:
        out.append(("block_edge_255_256", "order", swapped(sa, 255, 256, dtype)))
    if n > 700:
        out.append(("apart_500", "order", swapped(sa, 100, 600, dtype)))
    dup = sa.astype(dtype)
    dup[5] = dup[6]
    out.append(("duplicate", "order", dup))
    rng_cases = [("first_is_n", 0, n), ("last_is_n_plus_1", n - 1, n + 1), ("mid_is_u32_max", n // 2, 2 ** 32 - 1)]
    if width >= 5:
        rng_cases += [("mid_is_2_32", n // 2, 2 ** 32), ("mid_is_2_40_minus_1", n // 2, 2 ** 40 - 1)]
    if width == 8:
        rng_cases += [("mid_is_2_63", n // 2, 2 ** 63)]
    for name, r, v in rng_cases:
        a = sa.astype(dtype)
        a[r] = v
        out.append((name, "range", a))
    for _, _, a in out:
        a.setflags(write=False)
    return out


def by_name(cor):
    return {name: (kind, a) for name, kind, a in cor}


def pack40(a):
    """u64 values below 2^40 as packed little-endian 40-bit entries (sa_width = 5), 8 pad bytes."""
    a = np.ascontiguousarray(a, np.uint64)
    assert (a < 2 ** 40).all()
    b = a.view(np.uint8).reshape(-1, 8)[:, :5].reshape(-1)
    return np.concatenate([b, np.zeros(8, np.uint8)])


def touched(sa, a):
    """The ranks at which a differs from the true SA."""
    return np.flatnonzero(a.astype(np.uint64) != sa.astype(np.uint64))


def suffix_less(t, a, b):
    """Whole suffixes as byte strings: a proper prefix sorts first."""
    return bytes(t[a:]) < bytes(t[b:])


def unordered_pairs(t, a):
    """The ranks r whose pair (r - 1, r) is not strictly increasing, by brute force on the bytes."""
    return [r for r in range(1, len(a)) if not suffix_less(t, int(a[r - 1]), int(a[r]))]


def test_pack40_round_trip():
    a = np.array([0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 40 - 1, 0x123456789A], np.uint64)
    b = pack40(a)
    assert len(b) == 5 * len(a) + 8
    back = [int.from_bytes(bytes(b[5 * i:5 * i + 5]), "little") for i in range(len(a))]
    assert back == a.tolist()


def test_texts_are_what_the_catalogue_needs():
    t, sa, lcp = case("catalogue")
    n = len(t)
    assert 1900 <= n <= 2200 and t.max() <= 3
    assert O.check_sa(t, sa) == 0 and unordered_pairs(t, sa) == []
    by_char, by_len = pair_kinds(t, sa, lcp)
    assert int(lcp.max()) >= 200
    for d in DEPTHS:
        assert (by_char & (lcp == d)).any(), ("no char-decided pair at depth", d)
    for d in CATALOGUE_LEN_LCPS:
        assert (by_len & (lcp == d)).any(), ("no length-decided pair with lcp", d)
    assert by_len.sum() >= 70
    z, zsa, zlcp = case("zeros")
    assert len(z) == ZEROS_N and zsa.tolist() == list(range(ZEROS_N - 1, -1, -1))
    assert zlcp.tolist() == list(range(ZEROS_N))
    zc, zl = pair_kinds(z, zsa, zlcp)
    assert not zc.any() and zl[1:].all()


def test_catalogue_holds_every_shape():
    """By name, and from kasai_lcp of the true SA at the swapped rank: a change of the text or of the
    picker cannot silently empty a class."""
    for text, want_len, want_char in (("catalogue", CATALOGUE_LEN_LCPS, DEPTHS), ("zeros", ZEROS_LEN_LCPS, ())):
        t, sa, lcp = case(text)
        n = len(t)
        by_char, by_len = pair_kinds(t, sa, lcp)
        for width in (4, 5, 8):
            cor = by_name(corruptions(t, sa, width))
            assert all(a.dtype == (np.uint32 if width == 4 else np.uint64) and len(a) == n for _, a in cor.values())
            for d in want_char:
                kind, a = cor[f"char_lcp{d}"]
                r = touched(sa, a)
                assert kind == "order" and len(r) == 2 and r[1] == r[0] + 1 and lcp[r[1]] == d and by_char[r[1]]
            assert [k for k in cor if k.startswith("char_lcp")] == [f"char_lcp{d}" for d in want_char]
            for d in want_len:
                kind, a = cor[f"len_lcp{d}"]
                r = touched(sa, a)
                assert kind == "order" and len(r) == 2 and r[1] == r[0] + 1 and lcp[r[1]] == d and by_len[r[1]]
            if text == "zeros":   # rank = lcp there: the swaps sit at ranks 1, 32, 33, 64, 65 and 299
                assert [int(touched(sa, cor[f"len_lcp{d}"][1])[1]) for d in want_len] == list(want_len)
            assert touched(sa, cor["first_pair"][1]).tolist() == [0, 1]
            assert touched(sa, cor["last_pair"][1]).tolist() == [n - 2, n - 1]
            assert touched(sa, cor["duplicate"][1]).tolist() == [5] and cor["duplicate"][1][5] == sa[6]
            if text == "catalogue":
                assert touched(sa, cor["block_edge_255_256"][1]).tolist() == [255, 256]
                r = touched(sa, cor["apart_500"][1])
                assert len(r) == 2 and r[1] - r[0] == 500
            want_range = {"first_is_n": (0, n), "last_is_n_plus_1": (n - 1, n + 1), "mid_is_u32_max": (n // 2, 2 ** 32 - 1)}
            if width >= 5:
                want_range.update(mid_is_2_32=(n // 2, 2 ** 32), mid_is_2_40_minus_1=(n // 2, 2 ** 40 - 1))
            if width == 8:
                want_range.update(mid_is_2_63=(n // 2, 2 ** 63))
            assert {k for k, (kind, _) in cor.items() if kind == "range"} == set(want_range)
            for name, (r, v) in want_range.items():
                a = cor[name][1]
                assert touched(sa, a).tolist() == [r] and int(a[r]) == v and v >= n
            for name, (kind, a) in cor.items():
                if kind == "order":
                    assert int(a.max()) < n, name   # the safety rule of test_gpu_verify.py rests on this


def test_oracle_verdicts():
    """check_sa: 0 for the true SA, 2 for every swap, 1 for the duplicate and for every out-of-range
    entry (a u32 array holds all of width 4's)."""
    for text in ("catalogue", "zeros"):
        t, sa, _ = case(text)
        assert O.check_sa(t, sa) == 0
        for name, kind, a in corruptions(t, sa, 4):
            want = 1 if kind == "range" or name == "duplicate" else 2
            assert O.check_sa(t, a) == want, (text, name)
        for name, kind, a in corruptions(t, sa, 8):
            if kind == "order":
                assert O.check_sa(t, a.astype(np.uint32)) == (1 if name == "duplicate" else 2), (text, name)


def test_each_adjacent_swap_breaks_exactly_one_pair():
    """Brute force on the suffix bytes: after an adjacent swap the pair at the swapped rank is the
    only one out of order, so a verifier that misses it has nothing else to go by.  The swap of two
    ranks 500 apart breaks two pairs, the duplicate one (its two equal suffixes)."""
    for text in ("catalogue", "zeros"):
        t, sa, _ = case(text)
        for name, kind, a in corruptions(t, sa, 4):
            if kind != "order":
                continue
            r = touched(sa, a)
            bad = unordered_pairs(t, a)
            if name == "duplicate":
                assert bad == [6], (text, name, bad)
            elif name == "apart_500":
                assert bad == [r[0] + 1, r[1]], (text, name, bad)
            else:
                assert len(r) == 2 and bad == [r[1]], (text, name, bad)
