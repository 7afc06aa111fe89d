"""-m "not gpu": the numpy reference of the radix sort (tests/sort_checks.py) against typed-out cases, the result-index formula, and the
argument validation of emd_radix_sort (ABI 29), which needs no GPU: every call below fails before anything is launched."""
import ctypes as C

import numpy as np
import pytest

from emd_amd import _lib as L
from tests import sort_checks as sc

U = lambda *x: np.array(x, dtype=np.uint32)


def test_plain_sort_typed_out():
    keys = U(5, 3, 9, 3, 0, 7, 3, 1, 9)
    vals = U(10, 11, 12, 13, 14, 15, 16, 17, 18)
    k, v, count, word, idx = sc.sort_reference(keys, vals, passes=1, bits=4)
    assert k.tolist() == [0, 1, 3, 3, 3, 5, 7, 9, 9]
    assert v.tolist() == [14, 17, 11, 13, 16, 10, 15, 12, 18]            # the three 3s and the two 9s in input order
    assert (count, word, idx) == (9, 0, 1)
    # two passes of two bits order by the same four bits
    k2, v2, _, _, idx2 = sc.sort_reference(keys, vals, passes=2, bits=2)
    assert k2.tolist() == k.tolist() and v2.tolist() == v.tolist() and idx2 == 0


def test_high_bits_do_not_order():
    keys = U(0x13, 0x02, 0x21, 0x12, 0x01, 0x33, 0x22, 0x10)
    k, v, count, _, _ = sc.sort_reference(keys, np.arange(8, dtype=np.uint32), passes=1, bits=4)      # the low nibble alone
    assert [hex(x) for x in k] == ["0x10", "0x21", "0x1", "0x2", "0x12", "0x22", "0x13", "0x33"]
    assert v.tolist() == [7, 2, 4, 1, 3, 6, 0, 5] and count == 8
    k, v, _, _, _ = sc.sort_reference(keys, np.arange(8, dtype=np.uint32), passes=2, bits=4)
    assert k.tolist() == sorted(keys.tolist())


def test_compacting_drops_all_ones_and_values_are_indices():
    keys = U(8, 0xFFFFFFFF, 2, 8, 0xFFFFFFFF, 1, 2, 0xFFFFFFFE, 0)
    k, v, count, word, idx = sc.sort_reference(keys, passes=4, bits=8)
    assert k.tolist() == [0, 1, 2, 2, 8, 8, 0xFFFFFFFE]
    assert v.tolist() == [8, 5, 2, 6, 0, 3, 7]
    assert (count, word, idx) == (7, 0, 1)
    assert sc.sort_reference(keys, passes=4, bits=8, range_bits=27)[3] == 2          # 0xFFFFFFFE does not fit 27 bits
    assert sc.sort_reference(keys[:7], passes=4, bits=8, range_bits=27)[3] == 0      # the dropped keys never raise the word
    # everything dropped
    k, v, count, word, _ = sc.sort_reference(U(0xFFFFFFFF, 0xFFFFFFFF), passes=1, bits=8, range_bits=4)
    assert len(k) == len(v) == count == word == 0


def test_offset_wraps_and_raises_the_word():
    keys = U(105, 100, 99, 131, 100, 0xFFFFFFFF, 116, 104)
    k, v, count, word, idx = sc.sort_reference(keys, passes=2, bits=3, offset=100, range_bits=6)
    # rel = 5, 0, 2^32 - 1, 31, 0, -, 16, 4: the key below the offset wraps, sorts by its low six bits (63) and raises the word
    assert k.tolist() == [100, 100, 104, 105, 116, 131, 99]
    assert v.tolist() == [1, 4, 7, 0, 6, 3, 2]
    assert (count, word, idx) == (7, 2, 1)
    keys[2] = 163                                                                    # rel = 63 fits six bits
    assert sc.sort_reference(keys, passes=2, bits=3, offset=100, range_bits=6)[3] == 0
    keys[2] = 164                                                                    # rel = 64 = offset + 2^range_bits does not
    assert sc.sort_reference(keys, passes=2, bits=3, offset=100, range_bits=6)[3] == 2
    # a plain sort has no range check
    assert sc.sort_reference(keys, np.zeros(8, np.uint32), passes=2, bits=3, offset=100, range_bits=6)[3] == 0


def test_device_count_and_its_overflow_word():
    keys = U(4, 3, 2, 1, 0, 9, 9, 9)
    vals = U(0, 1, 2, 3, 4, 5, 6, 7)
    k, v, count, _, _ = sc.sort_reference(keys, vals, passes=1, bits=8, n_dev=4)
    assert k.tolist() == [1, 2, 3, 4] and v.tolist() == [3, 2, 1, 0] and count == 4
    k, v, count, _, idx = sc.sort_reference(keys, passes=3, bits=8, n_dev=5, n_dev_overflow=1)
    assert len(k) == len(v) == count == 0 and idx == 0
    assert sc.sort_reference(keys, vals, passes=1, bits=8, n_dev=0)[2] == 0


def test_result_index_formula():
    # emd_radix_result_buf (csrc/common.h), restated: pass 0 of a compacting sort writes pair 0, every other pass the pair it did not read
    expected = {(False, 0): 0, (False, 1): 1, (False, 2): 0, (False, 3): 1, (False, 4): 0,
                (True, 0): 0, (True, 1): 0, (True, 2): 1, (True, 3): 0, (True, 4): 1}
    for (compacting, passes), want in expected.items():
        assert sc.result_index(compacting, passes) == want, (compacting, passes)
        buf = 0                                                                      # the ping-pong walked pass by pass
        for p in range(passes):
            buf = 0 if (compacting and p == 0) else buf ^ 1
        assert buf == want


def test_failure_text_names_position_and_digits():
    with pytest.raises(AssertionError) as e:
        sc.assert_same("keys", U(*range(3000)), U(*range(2600), 7, *range(2601, 3000)), passes=2, bits=8, offset=1)
    msg = str(e.value)
    assert "position 2600 (sort block 1, wave slice 1, round 0, lane 40)" in msg and "key 0x00000007" in msg
    assert "pass 0: 6, pass 1: 0" in msg and "got 0x00000A28, expected 0x00000007" in msg
    sc.assert_same("keys", U(1, 2), U(1, 2))


def _args(**kw):
    one = 256                                                # a non-null pointer that is never dereferenced: validation fails first
    a = L.EmdRadixSortArgs()
    a.keys[0] = a.keys[1] = a.vals[0] = a.vals[1] = one
    a.hist = one
    a.n_cap, a.passes, a.bits, a.range_bits = 1000, 4, 8, 32
    for name, v in kw.items():
        if name in ("keys0", "keys1", "vals0", "vals1"):
            getattr(a, name[:4])[int(name[4])] = v
        else:
            setattr(a, name, v)
    return a


def test_symbol_exported_and_abi_29():
    lib = L.load()
    assert "emd_radix_sort" in L.EXPORTED_SYMBOLS and hasattr(lib, "emd_radix_sort")
    assert lib.emd_abi_version() == L.ABI_VERSION >= 29


@pytest.mark.parametrize("kw, text", [
    (dict(keys0=None), b"null"), (dict(keys1=None), b"null"), (dict(vals0=None), b"null"), (dict(vals1=None), b"null"), (dict(hist=None), b"null"),
    (dict(bits=0), b"bits"), (dict(bits=10), b"bits"), (dict(bits=-3), b"bits"),
    (dict(passes=-1), b"passes"), (dict(passes=5), b"passes"), (dict(passes=4, bits=9), b"passes"), (dict(passes=33, bits=1), b"passes"),
    (dict(keys_in=256, passes=0, count_out=256), b"compacting"), (dict(keys_in=256, passes=2), b"compacting"),
    (dict(range_bits=27), b"overflow_word"), (dict(keys_in=256, count_out=256, range_bits=27), b"overflow_word"),
    (dict(range_bits=-1, overflow_word=256), b"range_bits"), (dict(range_bits=33, overflow_word=256), b"range_bits"),
    (dict(n_dev_overflow=256), b"n_dev"),
    (dict(n_cap=-1), b"n_cap"), (dict(n_cap=2 ** 32), b"n_cap"), (dict(n_cap=2 ** 32 - 2048), b"n_cap"), (dict(n_cap=2 ** 40), b"n_cap"),
])
def test_invalid_arguments(kw, text):
    lib = L.load()
    assert lib.emd_radix_sort(C.byref(_args(**kw)), None) == L.EMD_ERR_INVALID, kw
    assert text in lib.emd_last_error(), (kw, lib.emd_last_error())


def test_null_args_and_empty_input():
    lib = L.load()
    assert lib.emd_radix_sort(None, None) == L.EMD_ERR_INVALID
    assert b"null" in lib.emd_last_error()
    # n_cap == 0: the result index, nothing launched (no GPU here to launch on)
    for passes in range(5):
        assert lib.emd_radix_sort(C.byref(_args(n_cap=0, passes=passes)), None) == sc.result_index(False, passes)
        if passes:
            assert lib.emd_radix_sort(C.byref(_args(n_cap=0, passes=passes, keys_in=256, count_out=256)), None) == sc.result_index(True, passes)
    assert lib.emd_radix_sort(C.byref(_args(n_cap=0, passes=3, bits=9, keys_in=256, count_out=256, range_bits=27, overflow_word=256)), None) == 0
