"""The cross-lane primitives of lld_slam_amd/csrc/lld_wave.h on their own, through the experiments build's lld_exp_wave_prims: one workgroup
over caller data, every result held bit for bit to a numpy model of the order the header documents."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

WP_SCAN, WP_SORT, WP_INT, WP_F64, WP_BLOCK, WP_HAMMING = range(6)
ONES = np.uint64(0xFFFFFFFFFFFFFFFF)


@pytest.fixture(scope="module")
def prims():
    from lld_slam_amd import Context, abi
    lib = abi.Lib(os.path.join(os.path.dirname(abi.product_library_path()), "liblld_amd_exp.so"), "lld_")
    fn = lib.fn("exp_wave_prims")
    fn.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]; fn.restype = C.c_int
    ctx = Context(0, lib=lib)

    def run(what, threads, n, data, out_bytes):
        data = np.ascontiguousarray(data)
        out = np.zeros(out_bytes, np.uint8)
        assert fn(ctx.handle, what, threads, n, data.ctypes.data, out.ctypes.data) == 0
        return out
    yield run
    ctx.close()


def butterfly(x, width, op):
    """What every lane holds after `x = op(x, x of lane ^ o)` for o = width/2, ..., 1."""
    x = np.array(x)
    lanes = np.arange(x.size)
    o = width // 2
    while o:
        x = op(x, x[lanes ^ o])
        o //= 2
    return x


def block_sum_model(x):
    """lld_wave::block_sum: the butterfly inside each wavefront, then 0 + the wavefront totals in ascending order."""
    t = x.dtype.type(0)
    for w in butterfly(x, 64, np.add)[::64]:
        t = t + w
    return t


# ---------------------------------------------------------------------------------------------------------------- scan

def scan_inputs(threads):
    rng = np.random.default_rng(threads)
    def single(i):
        v = np.zeros(threads, np.int32); v[i] = 1
        return v
    return {"zeros": np.zeros(threads, np.int32), "ones": np.ones(threads, np.int32), "random": rng.integers(0, 4, threads).astype(np.int32),
            "one_at_0": single(0), "one_at_63": single(63), "one_at_64": single(64), "one_at_last": single(threads - 1)}


@pytest.mark.parametrize("threads", [256, 1024])
@pytest.mark.parametrize("case", ["zeros", "ones", "random", "one_at_0", "one_at_63", "one_at_64", "one_at_last"])
def test_block_excl_scan(prims, threads, case):
    """Two different scans back to back through the same LDS array - the reuse the leading barrier exists for: `case`, then other random data."""
    a = scan_inputs(threads)[case]
    b = np.random.default_rng(7).integers(0, 4, threads).astype(np.int32)
    got = prims(WP_SCAN, threads, 0, np.stack([a, b]), 8 * (threads + 1)).view(np.int32).reshape(2, threads + 1)
    for g, v in zip(got, (a, b)):
        np.testing.assert_array_equal(g[:threads], np.cumsum(v) - v)
        assert g[threads] == v.sum()


# ---------------------------------------------------------------------------------------------------------------- sort

def sort_inputs(npad):
    rng = np.random.default_rng(npad)
    rnd = rng.integers(0, 2 ** 63, npad, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, npad, dtype=np.uint64)   # all 64 bits in use
    tail = rnd.copy(); tail[npad - npad // 3 - 1:] = ONES
    return {"random": rnd, "duplicates": rng.integers(0, 4, npad, dtype=np.uint64) << np.uint64(40), "sorted": np.sort(rnd), "reversed": np.sort(rnd)[::-1],
            "sentinel_tail": tail}


@pytest.mark.parametrize("npad", [2, 64, 128, 4096])
@pytest.mark.parametrize("case", ["random", "duplicates", "sorted", "reversed", "sentinel_tail"])
def test_bitonic_sort(prims, npad, case):
    """256 lanes: npad below and above the workgroup."""
    keys = sort_inputs(npad)[case]
    got = prims(WP_SORT, 256, npad, keys, 8 * npad).view(np.uint64)
    np.testing.assert_array_equal(got, np.sort(keys))


# ---------------------------------------------------------------------------------------------------------------- reductions

def int_inputs():
    rng = np.random.default_rng(11)
    rnd = rng.integers(-2 ** 31, 2 ** 31, 64).astype(np.int32)
    fill = np.full(64, np.iinfo(np.int32).max, np.int32)
    fill[[3, 17, 40, 41, 63]] = rng.integers(-2 ** 31, 2 ** 31, 5).astype(np.int32)
    return {"random": rnd, "int_max_fillers": fill}


@pytest.mark.parametrize("case", ["random", "int_max_fillers"])
def test_int_sum_min_max_at_every_width(prims, case):
    """Widths 64, 16, 8 and 4; every lane holds its group's result (the sums in the 32-bit wrap-around arithmetic of the adder)."""
    x = int_inputs()[case]
    got = prims(WP_INT, 64, 0, x, 4 * 4 * 3 * 64).view(np.int32).reshape(4, 3, 64)
    with np.errstate(over="ignore"):
        for wi, width in enumerate((64, 16, 8, 4)):
            groups = x.reshape(-1, width)
            exp_sum = np.repeat(groups.astype(np.int64).sum(1).astype(np.int32), width)
            np.testing.assert_array_equal(got[wi, 0], exp_sum, err_msg="sum<%d>" % width)
            np.testing.assert_array_equal(got[wi, 1], np.repeat(groups.min(1), width), err_msg="min<%d>" % width)
            np.testing.assert_array_equal(got[wi, 2], np.repeat(groups.max(1), width), err_msg="max<%d>" % width)


def f64_inputs():
    rng = np.random.default_rng(13)
    cancel = np.tile(np.array([1e16, 1.0, -1e16, 1.0]), 16)          # the last bit of the total depends on the order
    return {"random": rng.normal(size=(3, 64)) * 10.0 ** rng.integers(-8, 9, (3, 64)),
            "cancelling": np.stack([cancel, np.roll(cancel, 1), rng.permutation(cancel)])}


@pytest.mark.parametrize("case", ["random", "cancelling"])
def test_double_sum_is_the_xor_butterfly(prims, case):
    v = f64_inputs()[case]
    got = prims(WP_F64, 64, 0, v, 8 * 4 * 64).view(np.float64).reshape(4, 64)
    exp = [butterfly(r, 64, np.add) for r in v]
    if case == "cancelling":                                          # the case does what it is for: lane order gives another total (1, not 32)
        assert exp[0][0] != sum(v[0].tolist())
    np.testing.assert_array_equal(got[0].view(np.uint64), exp[0].view(np.uint64))
    for k in range(3):                                                # several values through one butterfly: the same bits as one at a time
        np.testing.assert_array_equal(got[1 + k].view(np.uint64), exp[k].view(np.uint64))
    np.testing.assert_array_equal(got[1].view(np.uint64), got[0].view(np.uint64))


@pytest.mark.parametrize("threads", [256, 768])
def test_block_sum_and_max(prims, threads):
    """Butterfly inside the wavefront, then the wavefront totals in ascending order; the second call reuses the first one's LDS array."""
    rng = np.random.default_rng(threads)
    x = rng.normal(size=threads) * 10.0 ** rng.integers(-6, 7, threads)
    x[::4] = np.tile(np.array([1e16, 1.0, -1e16, 1.0]), threads // 16)
    k = rng.integers(-2 ** 20, 2 ** 20, threads).astype(np.int32)
    got = prims(WP_BLOCK, threads, 0, np.concatenate([x.view(np.uint8), k.view(np.uint8)]), 20 * threads)
    s, m, ks = got[:8 * threads].view(np.float64), got[8 * threads:16 * threads].view(np.float64), got[16 * threads:].view(np.int32)
    np.testing.assert_array_equal(s.view(np.uint64), np.full(threads, block_sum_model(x)).view(np.uint64))
    np.testing.assert_array_equal(m, np.full(threads, np.abs(x).max()))
    np.testing.assert_array_equal(ks, np.full(threads, block_sum_model(k), np.int32))
    assert ks[0] == k.sum()


# ---------------------------------------------------------------------------------------------------------------- Hamming

def test_hamming256_all_overloads(prims):
    rng = np.random.default_rng(17)
    a = rng.integers(0, 2 ** 32, (69, 8), dtype=np.uint64).astype(np.uint32)
    b = rng.integers(0, 2 ** 32, (69, 8), dtype=np.uint64).astype(np.uint32)
    a[64] = 0; b[64] = 0xFFFFFFFF                                      # all-zero against all-one: 256
    b[65:] = a[65:]                                                   # identical pairs: 0
    got = prims(WP_HAMMING, 64, 69, np.concatenate([a, b], axis=1), 12 * 69).view(np.int32).reshape(3, 69)
    exp = np.unpackbits((a ^ b).view(np.uint8), axis=1).sum(1).astype(np.int32)
    assert exp[64] == 256 and not exp[65:].any()
    for g in got:
        np.testing.assert_array_equal(g, exp)
