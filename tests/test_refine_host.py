"""Host-only export of the refinement tables (phx_refine_tables) against the numpy specification.  No GPU is touched."""
import ctypes as C

import numpy as np
import pytest

import refine_ref as RR


def _tables(ctype):
    from phifem_amd import _lib as L
    nvpc = RR.NVPC[ctype]
    nepc = 0 if ctype == "quadrilateral" else len(RR.LOCAL_PAIRS[ctype])
    children = np.full((8, nvpc), -7, dtype=np.int32)
    w = np.full((8, max(nepc, 1), nvpc + nepc), np.nan)
    nchild = C.c_int(0)
    L.check(L.lib.phx_refine_tables(L.CELL_TYPES[ctype], children.ctypes.data_as(C.c_void_p), C.byref(nchild),
                                    w.ctypes.data_as(C.c_void_p)))
    n = nchild.value
    wflat = w.reshape(-1)[:n * nepc * (nvpc + nepc)].reshape(n, nepc, nvpc + nepc)
    return children.reshape(-1)[:n * nvpc].reshape(n, nvpc), wflat, children, w


@pytest.mark.parametrize("ctype", ["triangle", "tetrahedron", "quadrilateral"])
def test_child_table_equals_reference(ctype):
    got, _, raw, _ = _tables(ctype)
    ref = RR.child_table(ctype)
    assert got.shape == ref.shape and np.array_equal(got, ref)
    assert np.all(raw.reshape(-1)[ref.size:] == -7)            # nothing written past the table


@pytest.mark.parametrize("ctype", ["triangle", "tetrahedron"])
def test_p2_weights_equal_reference_and_are_dyadic(ctype):
    _, got, _, raw = _tables(ctype)
    ref = RR.p2_weight_table(ctype)
    assert got.shape == ref.shape
    assert np.array_equal(got, ref.astype(np.float64))
    assert all(float(f) == f for f in ref.reshape(-1))          # exactly representable
    assert np.array_equal(got * 8, np.round(got * 8))           # multiples of 1/8
    assert np.all(np.isnan(raw.reshape(-1)[ref.size:]))


def test_quadrilateral_writes_no_weights_and_other_cells_are_refused():
    from phifem_amd import _lib as L
    _, _, _, raw = _tables("quadrilateral")
    assert np.all(np.isnan(raw))
    n = C.c_int(0)
    L.check(L.lib.phx_refine_tables(L.TETRAHEDRON, None, C.byref(n), None))
    assert n.value == 8
    with pytest.raises(NotImplementedError):
        L.check(L.lib.phx_refine_tables(7, None, C.byref(n), None))
