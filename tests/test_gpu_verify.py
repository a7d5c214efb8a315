"""The SA verifier must refuse wrong arrays (SAS_BUILD_VERIFY, sas_verify: k_verify_adj<4 / 5 / 8>
and k_count_bits), and the intake of a caller's array (load_sa / k_convert_sa) must keep every
value and lose no out-of-range one before the check.  The wrong arrays are the catalogue of
tests/test_verify_host.py, whose verdicts the oracle gives there; every comparison here is exact
(accept or refuse, errno, equal arrays).

Safety rule of every case in this file.  A wrong array is input that the library is told to check,
never input that it is left to run on:

* an array with an entry >= n is only ever passed with verify=True: the range check then fails the
  build before any later stage reads text at an SA value (k_verify_adj itself tests a value before
  it reads text there, and load_sa tests the caller's value before narrowing it);
* builds without the flag take in-range corruptions only (swaps, one duplicate), and build nothing
  derived (BARE below).  What such a build runs over the SA is k_rel (the binary search's pivots:
  text reads at SA values, and at SA[mid] + P with P <= SAS_REL_PMAX = 24, inside the text's
  padding for any value < n), the shard's copy of SA[rank_hi] to the host (a value, never used as
  an address by the build), and for tagged=True k_tag_entries / k_tt_fill (text at SA values, and
  table slots bounded by the 4^p keys whatever the order): all in bounds for any in-range array;
* no corrupted index is ever searched: it is verified and freed.
"""
import errno

import numpy as np
import pytest

from test_verify_host import by_name, case, corruptions, pack40, touched

pytestmark = pytest.mark.gpu

BARE = dict(lcp=False, stree=False, sector=False, quad=False, llcp=False, prefix=False)
# the reduced set of the intake matrix: a char-decided swap at depth 64, a length-decided one,
# the duplicate and the smallest out-of-range value
REDUCED = ("char_lcp64", "len_lcp33", "duplicate", "first_is_n")
RANGE_MSG = ("entry >= n",)
ORDER_MSG = ("not sorted", "not a permutation")


@pytest.fixture(scope="module")
def sas():
    import sas_amd
    return sas_amd


def refused(sas, kind, call, what):
    """call() raises SasError EINVAL with the message of its kind."""
    with pytest.raises(sas.SasError) as e:
        idx = call()
        if idx is not None:   # only if the wrong array was accepted
            idx.free()
    assert e.value.code == errno.EINVAL, (what, str(e.value))
    msgs = RANGE_MSG if kind == "range" else ORDER_MSG
    assert any(m in str(e.value) for m in msgs), (what, str(e.value))


def stored(idx):
    sa = idx.suffix_array().astype(np.uint64)
    idx.free()
    return sa


# ---------------------------------------------------------------- a. verify at build
@pytest.mark.parametrize("width,sa40", [(4, False), (8, True)])
@pytest.mark.parametrize("text", ["catalogue", "zeros"])
def test_build_verify_refuses_the_catalogue(sas, text, width, sa40):
    """k_verify_adj<4> (host u32 array -> u32 index) and <5> (host u64 array -> 40-bit index) on
    every entry of the catalogue.  After each refusal a good build succeeds."""
    t, sa, _ = case(text)
    dtype = np.uint32 if width == 4 else np.uint64
    good = sa.astype(dtype)

    def build(a):
        return sas.SaNaive.build(t, sa=a, verify=True, sa40=sa40, **BARE)

    idx = build(good)
    assert idx.stats()["sa_width"] == (5 if sa40 else 4)
    assert np.array_equal(stored(idx), sa.astype(np.uint64))
    cor = corruptions(t, sa, width)
    assert len(cor) >= (26 if text == "catalogue" else 14)   # tests/test_verify_host.py says what they are
    for name, kind, a in cor:
        assert a.dtype == dtype
        refused(sas, kind, lambda: build(a), (text, width, name))
        build(good).free()


# ---------------------------------------------------------------- b. intake matrix
def raw_build(sas, t, sa_bytes, sa_width, flags, device):
    """sas_build itself (SaNaive.build derives the width from the element size, so it cannot say 5):
    text and SA as host arrays or as CUDA tensors."""
    import ctypes as C
    from sas_amd import _lib
    n = len(t)
    if device:
        import torch
        t = torch.from_numpy(np.array(t)).cuda()
        sa_bytes = torch.from_numpy(np.array(sa_bytes)).cuda()
        flags |= _lib.SAS_DEVICE_PTRS
        pt, ps = t.data_ptr(), sa_bytes.data_ptr()
    else:
        t, sa_bytes = np.ascontiguousarray(t), np.ascontiguousarray(sa_bytes)
        pt, ps = t.ctypes.data, sa_bytes.ctypes.data
    h = C.c_void_p()
    _lib.check(_lib.lib().sas_build(pt, n, ps, sa_width, flags, C.byref(h)))
    return sas.SaNaive(h, n)


def as_bytes(a, width):
    """A catalogue array (u32 for width 4, u64 for 5 and 8) as the caller's bytes."""
    if width == 5:
        return pack40(a)
    return np.ascontiguousarray(a, np.uint32 if width == 4 else np.uint64).view(np.uint8)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("sa40", [False, True], ids=["u32", "sa40"])
@pytest.mark.parametrize("width", [4, 5, 8])
def test_intake_matrix(sas, width, sa40, device):
    """Caller width x index width x pointer kind: the true SA is stored exactly (k_convert_sa<4,5>,
    <5,4>, <8,4>, <8,5> and the two plain copies), and the reduced set is refused."""
    from sas_amd import _lib
    t, sa, _ = case("catalogue")
    flags = _lib.SAS_BUILD_VERIFY | (_lib.SAS_BUILD_SA40 if sa40 else 0)
    dtype = np.uint32 if width == 4 else np.uint64
    idx = raw_build(sas, t, as_bytes(sa.astype(dtype), width), width, flags, device)
    assert idx.stats()["sa_width"] == (5 if sa40 else 4)
    assert np.array_equal(stored(idx), sa.astype(np.uint64))
    # and without the flag: the stored values do not depend on the check
    assert np.array_equal(stored(raw_build(sas, t, as_bytes(sa.astype(dtype), width), width,
                                           flags & ~_lib.SAS_BUILD_VERIFY, device)), sa.astype(np.uint64))
    cor = by_name(corruptions(t, sa, width))
    for name in REDUCED:
        kind, a = cor[name]
        refused(sas, kind, lambda: raw_build(sas, t, as_bytes(a, width), width, flags, device), (width, sa40, device, name))


# ---------------------------------------------------------------- c. truncation
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("width,sa40,add", [(8, False, 2 ** 32), (5, False, 2 ** 32), (8, True, 2 ** 40)],
                         ids=["u64_to_u32", "packed40_to_u32", "u64_to_sa40"])
def test_out_of_range_value_is_not_truncated_into_range(sas, width, sa40, add, device):
    """v + 2^32 (v + 2^40) narrows to the true entry v: the stored array would be the true SA.  The
    caller's own value is >= n and the build says so."""
    from sas_amd import _lib
    t, sa, _ = case("catalogue")
    flags = _lib.SAS_BUILD_VERIFY | (_lib.SAS_BUILD_SA40 if sa40 else 0)
    for r in (0, len(t) // 2, len(t) - 1):
        a = sa.astype(np.uint64)
        a[r] += add
        assert int(a[r]) % (2 ** (40 if sa40 else 32)) == int(sa[r])
        refused(sas, "range", lambda: raw_build(sas, t, as_bytes(a, width), width, flags, device), (width, sa40, r))


# ---------------------------------------------------------------- d. sas_verify on a built index
@pytest.mark.parametrize("sa40", [False, True], ids=["u32", "sa40"])
@pytest.mark.parametrize("text", ["catalogue", "zeros"])
def test_verify_on_a_built_index(sas, text, sa40):
    """Built without the flag from every in-range corruption, then idx.verify(): k_verify_adj<4>
    and <5> on the index's own array."""
    t, sa, _ = case(text)

    def build(a):
        return sas.SaNaive.build(t, sa=a, sa40=sa40, **BARE)

    idx = build(sa)
    idx.verify()
    idx.free()
    for name, kind, a in corruptions(t, sa, 4):
        if kind != "order":
            continue
        assert int(a.max()) < len(t)   # the safety rule
        idx = build(a)
        try:
            refused(sas, kind, idx.verify, (text, sa40, name))
        finally:
            idx.free()


def test_verify_on_a_tagged_index(sas):
    """k_verify_adj<8> on the 8-byte tagged entries.  Only char-decided swaps at depth >= 32: both
    suffixes share their bucket, so the bucket table is built from unchanged keys."""
    t, sa, _ = case("catalogue")

    def build(a, **kw):
        return sas.SaNaive.build(t, sa=a, tagged=True, **dict(BARE, **kw))

    idx = build(sa)
    assert idx.stats()["sa_width"] == 8 and idx.stats()["tag_chars"] < 32
    idx.verify()
    assert np.array_equal(stored(idx), sa.astype(np.uint64))
    cor = by_name(corruptions(t, sa, 4))
    for d in (32, 33, 63, 64, 65, 95, 96, 97, 200):
        kind, a = cor[f"char_lcp{d}"]
        idx = build(a)
        try:
            refused(sas, kind, idx.verify, ("tagged", d))
        finally:
            idx.free()
    # bucket lines hold no SA array to verify later: the check at build is the only one
    build(sa, tag_lines=True, verify=True).free()
    kind, a = cor["char_lcp64"]
    refused(sas, kind, lambda: build(a, tag_lines=True, verify=True), "tag_lines")


# ---------------------------------------------------------------- e. shards
@pytest.mark.parametrize("sa40", [False, True], ids=["u32", "sa40"])
def test_shard_checks(sas, sa40):
    """rank_range = (100, n - 5).  verify=True checks the caller's whole array, so a swap below rank
    100 is refused at build.  verify() on a built shard checks the ranks it holds: it refuses a
    wrong order inside them and accepts an array that is wrong only outside them, because the shard
    holds no such entry.  That acceptance is the documented reach of a shard's check (include/sas.h),
    not a guarantee about the caller's array."""
    t, sa, _ = case("catalogue")
    n = len(t)
    lo, hi = 100, n - 5

    def build(a, **kw):
        return sas.SaNaive.build(t, sa=a, rank_range=(lo, hi), sa40=sa40, **dict(BARE, **kw))

    idx = build(sa, verify=True)
    idx.verify()
    assert idx.stats()["rank_lo"] == lo and idx.stats()["next_pos"] == sa[hi]
    assert np.array_equal(stored(idx), sa[lo:hi].astype(np.uint64))
    inside = outside = 0
    for name, kind, a in corruptions(t, sa, 4):
        if kind != "order":
            continue
        refused(sas, kind, lambda: build(a, verify=True), ("shard build", name))
        r = touched(sa, a)
        idx = build(a)
        try:
            if r.min() >= lo and r.max() < hi:
                inside += 1
                refused(sas, kind, idx.verify, ("shard", name))
            elif r.max() < lo or r.min() >= hi:
                outside += 1
                idx.verify()
                assert np.array_equal(idx.suffix_array().astype(np.uint64), sa[lo:hi].astype(np.uint64))
        finally:
            idx.free()
    assert inside >= 10 and outside >= 3, (inside, outside)   # first_pair, last_pair, duplicate: outside


# ---------------------------------------------------------------- f. the second grid pass
def test_second_grid_pass(sas):
    """grid_for caps a launch at 2^18 blocks of 256 threads: above 2^26 entries k_verify_adj's
    grid-stride loop takes a second pass.  n = 2^26 + 1000; the library's own SA with the ranks
    (2^26 + 500, 2^26 + 501) swapped must be refused, the untouched one accepted, at build and by
    verify() on the shard of ranks [0, n - 1) built from them without the flag.  Text and SA stay
    on the device; the host reads the four entries and text windows around the swap, and checks from
    the text bytes that the swap puts exactly that pair out of order."""
    import torch
    from sas_amd import _lib
    n = (1 << 26) + 1000
    r = (1 << 26) + 501
    t = sas.random_string(n, seed=26, device="cuda")
    idx = sas.SaNaive.build(t, **BARE)
    dsa = torch.empty(n, dtype=torch.int32, device="cuda")
    _lib.check(_lib.lib().sas_copy_sa(idx._h, dsa.data_ptr(), n, _lib.SAS_DEVICE_PTRS))
    idx.free()
    torch.cuda.synchronize()
    a, b, c, d = (int(v) for v in dsa[r - 2:r + 2].cpu())   # ranks r - 2, r - 1, r, r + 1

    def suffix(p):   # 512 chars decide any pair of a random text; asserted below
        return bytes(t[p:p + 512].cpu().numpy())

    def less(x, y):
        sx, sy = suffix(x), suffix(y)
        assert sx != sy
        return sx < sy

    assert less(a, b) and less(b, c) and less(c, d)            # the true order, from the text
    assert less(a, c) and not less(c, b) and less(b, d)        # after the swap: only (c, b) is wrong

    def build(s):
        return sas.SaNaive.build(t, sa=s, verify=True, **BARE)

    def shard_verify(s):   # in range, so it may be built without the flag (the module's safety rule)
        idx = sas.SaNaive.build(t, sa=s, rank_range=(0, n - 1), **BARE)
        try:
            idx.verify()
        finally:
            idx.free()

    build(dsa).free()
    shard_verify(dsa)
    dsa[r - 1], dsa[r] = c, b
    torch.cuda.synchronize()
    refused(sas, "order", lambda: build(dsa), "second grid pass")
    # a whole index has the position count behind the compare (a pass that skipped ranks would leave
    # positions unseen); a shard's check of its 2^26 + 999 ranks has only the compare
    refused(sas, "order", lambda: shard_verify(dsa), "second grid pass, shard")
    # the same swap in the first pass is refused too (the case above is not refused for its size)
    dsa[r - 1], dsa[r] = b, c
    p, q = (int(v) for v in dsa[500:502].cpu())
    dsa[500], dsa[501] = q, p
    torch.cuda.synchronize()
    refused(sas, "order", lambda: build(dsa), "first grid pass")
