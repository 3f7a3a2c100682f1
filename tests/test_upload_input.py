"""What Engine.upload_v / Engine.upload_weights hand to the C side for every form of array a caller may pass (these tests run
without a GPU).  The engine is built with Engine.__new__ around a stub library that records (pointer, dtype, ld, row0, rows)
of each nmfx_upload_v / nmfx_upload_weights call and reads the block back from host memory with exactly those arguments --
`rows` rows of n elements, `ld` elements apart, as copy_rows_in (engine.hip) reads it.  The block read that way must be the
array the caller passed, and ld >= n (the C side refuses anything less)."""
import ctypes as C

import numpy as np
import pytest
from numpy.lib.stride_tricks import sliding_window_view

from nmf_amd import _lib as L
from nmf_amd.engine import Engine

N = 7           # columns of the block
ROWS = 6


class StubLib:
    """nmfx_upload_v / nmfx_upload_weights of a library without a device: each call is recorded with the block it describes."""

    def __init__(self, n):
        self.n = n
        self.calls = []

    def _take(self, name, h, ptr, dtype, ld, row0, rows):
        ctype, npt = {L.F32: (C.c_float, np.float32), L.F64: (C.c_double, np.float64)}[dtype]
        block = np.empty((rows, self.n), dtype=npt)
        addr = C.cast(ptr, C.c_void_p).value
        for r in range(rows):
            block[r] = np.ctypeslib.as_array((ctype * self.n).from_address(addr + r * ld * C.sizeof(ctype)))
        self.calls.append(dict(name=name, dtype=dtype, ld=ld, row0=row0, rows=rows, block=block))
        return 0

    def nmfx_upload_v(self, *a):
        return self._take("v", *a)

    def nmfx_upload_weights(self, *a):
        return self._take("weights", *a)

    def nmfx_last_error(self, h):
        return b""


def engine(n=N, m=64, k=4):
    eng = Engine.__new__(Engine)
    eng.lib = StubLib(n)
    eng.m, eng.n, eng.k = m, n, k
    eng.h = None            # (close() has nothing to destroy)
    eng.precision_epoch = 0
    return eng


def _base(dtype, rows=2 * ROWS, cols=N + 5):
    return (np.random.default_rng(11).uniform(0.1, 1.0, (rows, cols)) * 8).astype(dtype)


FORMS = {
    "contiguous": lambda dt: np.ascontiguousarray(_base(dt)[:ROWS, :N]),
    "columns_of_wider": lambda dt: _base(dt)[:ROWS, :N],
    "every_second_row": lambda dt: _base(dt)[::2, :N],
    "fortran": lambda dt: np.asfortranarray(_base(dt)[:ROWS, :N]),
    "reversed_rows": lambda dt: _base(dt)[:ROWS, :N][::-1],
    "broadcast_row": lambda dt: np.broadcast_to(_base(dt)[0, :N], (ROWS, N)),
    "sliding_window": lambda dt: sliding_window_view(_base(dt).ravel()[:ROWS + N - 1], N),
}
METHODS = ("upload_v", "upload_weights")
DTYPES = (np.float32, np.float64)


def _upload(method, a, row0=3):
    eng = engine()
    getattr(eng, method)(a, row0=row0)
    (call,) = eng.lib.calls
    assert call["name"] == ("v" if method == "upload_v" else "weights")
    return call


def _check(call, a, dtype, row0=3):
    want = np.array(a, dtype=dtype)                 # a copy: what the caller's view shows
    assert call["dtype"] == (L.F32 if dtype == np.float32 else L.F64)
    assert call["rows"] == want.shape[0] and call["row0"] == row0
    assert call["ld"] >= N, call["ld"]
    assert call["block"].dtype == dtype
    assert np.array_equal(call["block"], want)


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("form", list(FORMS))
def test_block_reaches_the_c_side_as_the_caller_sees_it(form, dtype, method):
    a = FORMS[form](dtype)
    assert a.shape == (ROWS, N) and a.dtype == dtype
    _check(_upload(method, a), a, dtype)


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("form", list(FORMS))
def test_one_row_block_of_every_form(form, dtype, method):
    """A block of one row has no row stride to speak of: whatever strides[0] of the view says, the C side gets ld >= n."""
    a = FORMS[form](dtype)[2:3]
    assert a.shape == (1, N)
    _check(_upload(method, a), a, dtype)


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_one_row_with_an_arbitrary_row_stride(dtype, method):
    base = _base(dtype)
    for stride in (0, 1, 3, -5):                    # in elements: nothing a C reader could step by
        a = np.lib.stride_tricks.as_strided(base.ravel()[20:], shape=(1, N), strides=(stride * base.itemsize, base.itemsize))
        _check(_upload(method, a), a, dtype)


@pytest.mark.parametrize("method", METHODS)
def test_views_that_qualify_are_passed_without_a_copy(method):
    """The two strided forms the C side reads as they are keep their leading dimension: no copy of a large V on the way."""
    base = _base(np.float32)
    assert _upload(method, base[:ROWS, :N])["ld"] == N + 5
    assert _upload(method, base[::2, :N])["ld"] == 2 * (N + 5)
    assert _upload(method, np.ascontiguousarray(base[:ROWS, :N]))["ld"] == N


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("dtype", [np.int32, np.float16], ids=["int32", "float16"])
def test_other_dtypes_are_converted_to_float64(dtype, method):
    a = (np.random.default_rng(5).uniform(0, 50, (ROWS, N))).astype(dtype)
    _check(_upload(method, a), a, np.float64)
    _check(_upload(method, a[::-1][:, :N]), a[::-1], np.float64)


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("shape", [(ROWS, N + 1), (ROWS, N - 1), (N,), (2, ROWS, N)])
def test_wrong_column_count_raises(shape, method):
    eng = engine()
    with pytest.raises(ValueError, match="wrong shape"):
        getattr(eng, method)(np.ones(shape, dtype=np.float32))
    assert not eng.lib.calls
