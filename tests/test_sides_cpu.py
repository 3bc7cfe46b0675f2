"""taichislam_amd/mapping/_sides.py without a GPU and without the library: the host side's outputs and pointers, record_columns against the numpy view of
the same bytes and against the columns the wrappers used to spell out, and the table of device dtypes on torch builds with and without unsigned types."""
import types

import numpy as np
import pytest
import torch

from taichislam_amd.mapping import _sides
from taichislam_amd.mapping.dense_tsdf import PATH_SCORE_DTYPE, TRAJ_SCORE_DTYPE

KINDS = ("u1", "i2", "u2", "i4", "u4", "i8", "f4")


def test_host_out_is_the_dtype_asked_for_contiguous_and_zeroed():
    for kind in KINDS:
        for shape in (0, 5, (3, 4), (2, 0, 3), (2, 3, 5)):
            a = _sides.HOST.out(shape, kind)
            assert isinstance(a, np.ndarray) and a.dtype == np.dtype(kind) and a.shape == (shape if isinstance(shape, tuple) else (shape,)), (kind, shape)
            assert a.flags.c_contiguous and a.flags.writeable and not a.any()
            assert _sides.HOST.out(shape, kind, zero=True).dtype == a.dtype
    a = np.arange(4, dtype=np.uint8)
    assert _sides.HOST.put(a) is a


def test_ptr_of_none_is_none():
    assert _sides.HOST.ptr(None) is None and _sides._Device.ptr(None) is None and _sides._vp(None) is None
    a = np.zeros(3, np.float32)
    assert _sides.HOST.ptr(a).value == a.ctypes.data
    t = torch.zeros(3)
    assert _sides._Device.ptr(t) == t.data_ptr()


def _block(dtype, n, seed):
    """random int32 record blocks whose int64 fields hold a value above 2^32 and a negative one"""
    rng = np.random.default_rng(seed)
    block = rng.integers(-(1 << 31), 1 << 31, (n, dtype.itemsize // 4), dtype=np.int64).astype(np.int32)
    rows = block.view(dtype).reshape(n)
    for k in dtype.names:
        if dtype.fields[k][0].itemsize == 8 and n >= 2:
            rows[k][0], rows[k][1] = (1 << 32) + 12345, -7 - (1 << 33)
    return block


@pytest.mark.parametrize("dtype", [PATH_SCORE_DTYPE, TRAJ_SCORE_DTYPE], ids=["path", "traj"])
@pytest.mark.parametrize("n", [0, 1, 3, 257])
def test_record_columns_equal_the_numpy_view_of_the_same_bytes(dtype, n):
    block = _block(dtype, n, n + 1)
    want = block.view(dtype).reshape(n)
    got = _sides.record_columns(torch.from_numpy(block.copy()), dtype)
    host = _sides.record_columns(block, dtype)
    assert list(got) == list(dtype.names) == list(host)
    wide = [k for k in dtype.names if dtype.fields[k][0].itemsize == 8]
    assert wide and all(k.startswith("cost") for k in wide)
    for k in dtype.names:
        g = got[k].numpy()
        assert g.shape == (n,) and g.dtype == want[k].dtype and host[k].dtype == want[k].dtype, k
        assert g.tobytes() == want[k].tobytes() == host[k].tobytes(), k             # bit for bit: the float field too, whatever NaN its bits spell
        assert not np.shares_memory(host[k], block)
    if n >= 2:
        for k in wide:
            assert got[k][0].item() == (1 << 32) + 12345 and got[k][1].item() == -7 - (1 << 33)
    assert got["min_dist"].dtype == torch.float32


def test_record_columns_read_the_columns_the_wrappers_spelled_out():
    """score_paths read min_dist from column 6 and cost from columns 8:10; the trajectory records min_dist from 5, cost_collision from 8:10 and
    cost_smooth from 10:12; the first eight names were columns 0 .. 7"""
    for dtype, f32, i64 in ((PATH_SCORE_DTYPE, 6, {"cost": (8, 10)}), (TRAJ_SCORE_DTYPE, 5, {"cost_collision": (8, 10), "cost_smooth": (10, 12)})):
        rec = torch.from_numpy(_block(dtype, 9, 4))
        got = _sides.record_columns(rec, dtype)
        assert rec.shape[1] == {40: 10, 48: 12}[dtype.itemsize]
        for i, k in enumerate(dtype.names[:8]):
            want = rec[:, i].view(torch.float32) if i == f32 else rec[:, i]
            assert dtype.names[f32] == "min_dist" and got[k].dtype == want.dtype and got[k].numpy().tobytes() == want.numpy().tobytes(), k
        for k, (a, b) in i64.items():
            assert torch.equal(got[k], rec[:, a:b].contiguous().view(torch.int64).reshape(9)), k
        assert set(got) == set(dtype.names[:8]) | set(i64)


def test_device_dtypes_with_and_without_unsigned_types():
    names = ("uint8", "int16", "int32", "int64", "float32")
    full = types.SimpleNamespace(**{k: k for k in names}, uint16="uint16", uint32="uint32")
    bare = types.SimpleNamespace(**{k: k for k in names})
    width = {"uint8": 1, "int16": 2, "uint16": 2, "int32": 4, "uint32": 4, "int64": 8, "float32": 4}
    for ns in (full, bare):
        table = _sides.device_dtypes(ns)
        assert set(table) == set(KINDS)
        for kind, dt in table.items():
            assert width[dt] == np.dtype(kind).itemsize, (kind, dt)
    assert _sides.device_dtypes(full)["u2"] == "uint16" and _sides.device_dtypes(full)["u4"] == "uint32"
    assert _sides.device_dtypes(bare)["u2"] == "int16" and _sides.device_dtypes(bare)["u4"] == "int32"
    real = _sides.device_dtypes(torch)                                               # and on this torch: every kind a dtype of the kind's width
    for kind in KINDS:
        assert torch.empty(0, dtype=real[kind]).element_size() == np.dtype(kind).itemsize
