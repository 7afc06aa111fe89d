"""-m gpu: the stable LSD radix sort behind the depth sort, the tile sort and the k-NN lists, called directly (emd_radix_sort, ABI 29) on the
inputs where a ballot-ranked, LDS-reordered radix pass can go wrong, against the numpy reference of tests/sort_checks.py (pinned by
tests/test_sort_cpu.py, written from csrc/radix_sort.h).

Everything is integer and deterministic: every comparison is exact and covers every position of every buffer.  For every call `_sort_and_check`
asserts (a) the returned pair index, (b) keys / values of the result against the reference, (c) that nothing past the element count was
written in any of the four buffers, (d) the 4096-word guards behind keys[2], vals[2], hist and the device words, (e) *count_out and the
overflow word.  A failure names the first differing position, its sort block / wave slice / ballot round / lane, its key and the digit of
every pass.  Sizes are the smallest at which each mechanism exists: 64 keys per ballot round, 512 per wave slice, 2048 per sort block, 1024
block counts per trip of the digit scan."""
import ctypes as C

import numpy as np
import pytest
import torch

from emd_amd import _lib as L
from tests import sort_checks as sc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = 0xDEADBEEF             # pre-fill of every buffer and guard: never a key or a value of an input
GUARD = 4096
DEPTH_OFFSET = 0x3E4CCCCD     # the bits of 0.2f: the near plane of the narrow depth sort (bits 9, passes 3, range_bits 27)


def _to_dev(words, head=None):
    """`words` + GUARD words on the device, all SENT but for the leading `head`; -> (tensor, its initial contents)."""
    init = np.full(words + GUARD, SENT, dtype=np.uint32)
    if head is not None:
        init[:len(head)] = head
    return torch.from_numpy(init.view(np.int32)).to(DEV), init


def _host(t):
    return t.cpu().numpy().view(np.uint32)


def _sort_and_check(keys, vals=None, *, passes, bits, offset=0, range_bits=32, n_dev=None, n_dev_overflow=None, label=""):
    """One emd_radix_sort call on the current stream, checked in full; vals None: a compacting sort of `keys`.  -> the four buffers (host)."""
    keys = np.ascontiguousarray(keys, dtype=np.uint32)
    compacting, n_cap = vals is None, len(keys)
    assert not (keys == SENT).any() and (compacting or not (np.asarray(vals) == SENT).any()), "the sentinel occurs in the input"
    geometry = dict(passes=passes, bits=bits, offset=offset)
    label = f"{label} [{'compacting' if compacting else 'plain'} n_cap={n_cap} n_dev={n_dev}/{n_dev_overflow} passes={passes} bits={bits} offset=0x{offset:X} range_bits={range_bits}]"
    ref_k, ref_v, count, ref_word, ref_idx = sc.sort_reference(keys, vals, passes=passes, bits=bits, offset=offset, range_bits=range_bits, n_dev=n_dev,
                                                               n_dev_overflow=n_dev_overflow or 0)
    n = 0 if (n_dev is not None and n_dev_overflow) else (n_cap if n_dev is None else n_dev)

    bufs = {}
    bufs["keys0"] = _to_dev(n_cap, None if compacting else keys)
    bufs["vals0"] = _to_dev(n_cap, None if compacting else vals)
    bufs["keys1"], bufs["vals1"] = _to_dev(n_cap), _to_dev(n_cap)
    bufs["hist"] = _to_dev((512 if bits == 9 else 256) * ((n_cap + sc.SORT_TILE - 1) // sc.SORT_TILE))
    # device words: [0] count_out, [1] the overflow word, [2] *n_dev, [3] *n_dev_overflow, then a guard
    bufs["words"] = _to_dev(4, np.array([SENT, 0, n_dev or 0, n_dev_overflow or 0], dtype=np.uint32))
    keys_in = torch.from_numpy(keys.view(np.int32)).to(DEV) if compacting else None
    t = {name: b[0] for name, b in bufs.items()}

    a = L.EmdRadixSortArgs()
    a.keys_in = keys_in.data_ptr() if compacting else None
    a.keys[0], a.keys[1], a.vals[0], a.vals[1], a.hist = (t[x].data_ptr() for x in ("keys0", "keys1", "vals0", "vals1", "hist"))
    a.n_cap, a.passes, a.bits, a.offset, a.range_bits = n_cap, passes, bits, offset, range_bits
    w = t["words"].data_ptr()
    a.count_out, a.overflow_word = w, w + 4
    a.n_dev = w + 8 if n_dev is not None else None
    a.n_dev_overflow = w + 12 if n_dev_overflow is not None else None
    idx = L.load().emd_radix_sort(C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert idx >= 0, f"{label}: {L.load().emd_last_error()}"
    got = {name: _host(x) for name, x in t.items()}           # (the copies synchronise with the stream)

    # (d) every guard, (e) the device words
    for name, (_, init) in bufs.items():
        sc.assert_same(f"{label}: guard behind {name}", got[name][-GUARD:], init[-GUARD:])
    words = got["words"]
    assert idx == ref_idx, f"{label}: (a) returned pair {idx}, expected {ref_idx}"
    assert words[1] == ref_word, f"{label}: (e) overflow word {words[1]}, expected {ref_word}"
    assert words[2] == (n_dev or 0) and words[3] == (n_dev_overflow or 0), f"{label}: the device-side count was written to"
    if compacting:
        assert np.array_equal(_host(keys_in), keys), f"{label}: keys_in was written to"
    if ref_word:
        return got                                            # out of range: the callers discard this result, only the word and the guards are defined
    assert words[0] == (count if compacting else SENT), f"{label}: (e) count_out 0x{words[0]:X}, expected {count if compacting else 'untouched'}"
    # (b) the result, every position
    sc.assert_same(f"{label}: (b) keys[{idx}]", got[f"keys{idx}"][:count], ref_k, **geometry)
    sc.assert_same(f"{label}: (b) vals[{idx}]", got[f"vals{idx}"][:count], ref_v, report_keys=ref_k, **geometry)
    # (c) nothing behind the count: the pre-fill (compacting; pair 1 of a plain sort) or the caller's own pairs (pair 0 of a plain sort)
    for name in ("keys0", "vals0", "keys1", "vals1"):
        sc.assert_same(f"{label}: (c) {name} past the count", got[name][count:n_cap], bufs[name][1][count:n_cap])
    if passes == 0:
        for name in ("keys0", "vals0", "keys1", "vals1"):
            sc.assert_same(f"{label}: {name} of a sort without passes", got[name], bufs[name][1])
    assert compacting or count == n
    return got


# ---- key distributions --------------------------------------------------------------------------------------------------------------------
DISTRIBUTIONS = ("uniform", "equal", "alternate_by_lane", "alternate_by_64", "distinct_in_round", "ascending", "descending", "eight_values",
                 "top_digit_only", "digits_zero", "digits_max")


def _keys(dist, n, bits, passes, rng):
    """-> (keys [n] uint32, offset).  The digits meant are those of rel = key - offset."""
    i = np.arange(n, dtype=np.uint64)
    width, offset = passes * bits, 0
    a, b = 0x13579BDF, 0xECA86420                              # complements: they differ in every digit of every width
    if dist == "uniform":
        rel = rng.integers(0, 1 << 32, n, dtype=np.uint64)
    elif dist == "equal":
        rel = np.full(n, 0x9E3779B1, dtype=np.uint64)
    elif dist == "alternate_by_lane":
        rel = np.where(i & 1, a, b).astype(np.uint64)
    elif dist == "alternate_by_64":
        rel = np.where((i >> 6) & 1, a, b).astype(np.uint64)
    elif dist == "distinct_in_round":
        # the 64 keys of a ballot round carry the 64 lane numbers (rotated from round to round) in the top pass's digit, noise in all other bits
        shift = min((passes - 1) * bits, 26)
        lane = (i + (i >> 6)) & 63
        rel = (rng.integers(0, 1 << 32, n, dtype=np.uint64) & ~np.uint64(63 << shift)) | (lane << np.uint64(shift))
    elif dist in ("ascending", "descending"):
        rel = i * np.uint64((0xFFFFFFF0 // n) | 1)             # (an odd step: every digit of every pass varies)
        rel = rel[::-1].copy() if dist == "descending" else rel
    elif dist == "eight_values":
        rel = rng.integers(0, 1 << 32, 8, dtype=np.uint64)[rng.integers(0, 8, n)]
    elif dist == "top_digit_only":
        # every lower pass is all ties; the top pass must keep what they (did not) reorder
        rel = np.uint64(0x00ABCDEF & ((1 << ((passes - 1) * bits)) - 1)) | (rng.integers(0, 1 << bits, n, dtype=np.uint64) << np.uint64((passes - 1) * bits))
    else:
        # every sorted digit 0 / 2^bits - 1, noise above the sorted bits; an offset, so that all-ones rel is not the dropped key
        offset = 0x00012345
        low = 0 if dist == "digits_zero" else (1 << width) - 1
        rel = ((rng.integers(0, 1 << 32, n, dtype=np.uint64) << np.uint64(width)) & np.uint64(0xFFFFFFFF)) | np.uint64(low)
    keys = ((rel + np.uint64(offset)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    keys[(keys == SENT) | (keys == sc.DROPPED)] -= 1           # (never by design; by chance at most)
    return keys, offset


def _values(n, rng):
    return rng.permutation(n).astype(np.uint32)                # distinct: a stability error cannot hide behind equal values


@pytest.mark.parametrize("compacting", [False, True], ids=["plain", "compacting"])
def test_sizes_on_every_seam(compacting):
    """One ballot round, one wave slice, one block, ragged last blocks: 1 .. 6143 keys, four passes of eight bits."""
    rng = np.random.default_rng(100 + compacting)
    for n in (1, 63, 64, 65, 511, 512, 513, 2047, 2048, 2049, 4097, 6143):
        for dist in ("uniform", "equal", "eight_values"):
            keys, offset = _keys(dist, n, 8, 4, rng)
            if compacting:
                keys[rng.random(n) < 0.25] = sc.DROPPED
            _sort_and_check(keys, None if compacting else _values(n, rng), passes=4, bits=8, offset=offset, label=f"{dist} n={n}")


@pytest.mark.parametrize("compacting", [False, True], ids=["plain", "compacting"])
@pytest.mark.parametrize("bits", [1, 5, 8, 9])
def test_distributions_widths_and_pass_counts(bits, compacting):
    """Every distribution at 65 / 513 / 2049 / 6143 keys, passes 1..4 (1..3 of nine bits: the 512-bin kernels, bins >= 256 populated): both
    parities of the result index in both modes."""
    rng = np.random.default_rng(200 + 10 * bits + compacting)
    for passes in range(1, 4 if bits == 9 else 5):
        for dist in DISTRIBUTIONS:
            for n in (65, 513, 2049, 6143):
                keys, offset = _keys(dist, n, bits, passes, rng)
                if bits == 9 and dist in ("uniform", "ascending", "digits_max"):
                    assert ((((keys.astype(np.int64) - offset) & 0xFFFFFFFF) & 511) >= 256).any()
                if compacting:
                    keys[rng.random(n) < 0.125] = sc.DROPPED
                _sort_and_check(keys, None if compacting else _values(n, rng), passes=passes, bits=bits, offset=offset, label=f"{dist} n={n}")


def test_no_passes_leaves_pair_0_untouched():
    rng = np.random.default_rng(300)
    keys, _ = _keys("uniform", 2049, 8, 4, rng)
    _sort_and_check(keys, _values(2049, rng), passes=0, bits=8, label="passes=0")


@pytest.mark.parametrize("blocks", [1024, 2048])
@pytest.mark.parametrize("dist", ["uniform", "equal"])
def test_digit_scan_carries_across_1024_block_trips(blocks, dist):
    """blocks * 2048 + 1 keys: 1025 / 2049 sort blocks, so the per-digit scan over the block counts makes a second / third trip with a carry.
    uniform: a plain sort, two passes of eight bits; all equal: a compacting sort, three passes of nine bits, first and last key dropped."""
    n = blocks * 2048 + 1
    rng = np.random.default_rng(400 + blocks)
    keys, _ = _keys(dist, n, 8, 2, rng)
    if dist == "uniform":
        _sort_and_check(keys, _values(n, rng), passes=2, bits=8, label=f"uniform n={n}")
    else:
        keys[0] = keys[-1] = sc.DROPPED
        _sort_and_check(keys, passes=3, bits=9, label=f"equal n={n}")


def test_compaction_patterns():
    """Dropped fraction 0 / a half / all but one / all, dropped runs that cover exactly one sort block and exactly one wave slice, first and
    last element dropped; the values are the original indices (the reference's)."""
    n = 6143
    rng = np.random.default_rng(500)
    patterns = {
        "none": np.zeros(n, bool),
        "half": rng.random(n) < 0.5,
        "all_but_one": np.arange(n) != 3000,
        "all": np.ones(n, bool),
        "whole_block_1": (np.arange(n) >= 2048) & (np.arange(n) < 4096),
        "wave_slice_5": (np.arange(n) >= 2560) & (np.arange(n) < 3072),
        "first_and_last": (np.arange(n) == 0) | (np.arange(n) == n - 1),
    }
    for name, drop in patterns.items():
        for bits, passes in ((8, 1), (8, 2), (8, 4), (9, 3)):
            for dist in ("uniform", "eight_values"):
                keys, offset = _keys(dist, n, bits, passes, rng)
                keys[drop] = sc.DROPPED
                _sort_and_check(keys, passes=passes, bits=bits, offset=offset, label=f"drop {name}, {dist}")


def _depth_keys(n, rng):
    depth = np.exp(rng.uniform(np.log(0.2), np.log(1000.0), n)).astype(np.float32).clip(np.float32(0.2), np.float32(1000.0))
    depth[:2] = (0.2, 1000.0)
    return depth.view(np.uint32).copy()


def test_narrow_depth_sort_offset_and_range():
    """The narrow depth sort's configuration: offset = bits of 0.2f, three passes of nine bits, 27 bits of range, float-bit keys of depths in
    [0.2, 1000]: in range, the word stays exactly 0.  One kept key at offset + 2^27, or below the offset (it wraps), raises it to 2; the same
    position holding the dropped key does not."""
    cfg = dict(passes=3, bits=9, offset=DEPTH_OFFSET, range_bits=27)
    rng = np.random.default_rng(600)
    for n in (65, 2049, 6143):
        keys = _depth_keys(n, rng)
        assert keys.min() == DEPTH_OFFSET and ((keys.astype(np.int64) - DEPTH_OFFSET) >> 27).max() == 0
        keys[rng.random(n) < 0.25] = sc.DROPPED
        keys[:2] = (DEPTH_OFFSET, 0x447A0000)
        _sort_and_check(keys, **cfg, label=f"depths in range n={n}")
        at = n // 2 + 1
        for bad, word in ((DEPTH_OFFSET + (1 << 27), 2), (DEPTH_OFFSET - 1, 2), (0, 2), (DEPTH_OFFSET + (1 << 27) - 1, 0), (sc.DROPPED, 0)):
            k = keys.copy()
            k[at] = bad
            assert sc.sort_reference(k, **cfg)[3] == word
            _sort_and_check(k, **cfg, label=f"key 0x{bad:08X} at {at}, n={n}")
    # a plain sort with an offset has no range check and never touches the word
    keys = _depth_keys(2049, rng)
    keys[7] = DEPTH_OFFSET - 1
    _sort_and_check(keys, _values(2049, rng), **cfg, label="plain sort with an offset")


@pytest.mark.parametrize("compacting", [False, True], ids=["plain", "compacting"])
def test_device_side_count_below_capacity(compacting):
    """n_cap = 10 000 with the count on the device: 0, 1, one block, two blocks and one key, the capacity; and a count voided by its overflow
    word, after which nothing is written anywhere and a compacting sort publishes a count of 0."""
    n_cap = 10_000
    rng = np.random.default_rng(700 + compacting)
    for passes in (2, 3):
        for n_dev, ovf in ((0, None), (1, None), (2048, 0), (4097, None), (10_000, 0), (5000, 1)):
            keys, _ = _keys("uniform", n_cap, 8, passes, rng)
            if compacting:
                keys[rng.random(n_cap) < 0.25] = sc.DROPPED
            got = _sort_and_check(keys, None if compacting else _values(n_cap, rng), passes=passes, bits=8, n_dev=n_dev, n_dev_overflow=ovf,
                                  label=f"n_dev={n_dev}")
            if ovf:
                assert (got["keys1"] == SENT).all() and (got["vals1"] == SENT).all()
                assert got["words"][0] == (0 if compacting else SENT)


def test_same_bits_twice_and_on_a_side_stream():
    rng = np.random.default_rng(800)
    keys, _ = _keys("eight_values", 6143, 8, 4, rng)
    vals = _values(6143, rng)
    first = _sort_and_check(keys, vals, passes=4, bits=8, label="run 1")
    second = _sort_and_check(keys, vals, passes=4, bits=8, label="run 2")
    for name in ("keys0", "vals0", "keys1", "vals1"):
        assert np.array_equal(first[name], second[name]), name
    keys[rng.random(6143) < 0.5] = sc.DROPPED
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        assert torch.cuda.current_stream().cuda_stream == side.cuda_stream != 0
        third = _sort_and_check(keys, passes=3, bits=9, label="side stream")
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    fourth = _sort_and_check(keys, passes=3, bits=9, label="default stream")
    for name in ("keys0", "vals0", "keys1", "vals1"):
        assert np.array_equal(third[name], fourth[name]), name
