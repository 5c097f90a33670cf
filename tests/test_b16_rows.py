"""The host side of the 16-bit operand contract (odx.backend.rows16_operand: 16-byte aligned base, row stride a multiple of
64 elements, columns D .. stride zero) and the storage round trip of a model whose centres are 16-bit.  No GPU."""
import numpy as np
import pytest
import torch

import odx
from odx import storage
from odx.backend import B16_DTYPES, Features, HipBackend, rows16_operand
from tests.oracle_backend import OracleBackend


@pytest.mark.parametrize("dtype", B16_DTYPES)
@pytest.mark.parametrize("n,D", [(5, 36), (3, 64), (7, 65), (2, 1000), (1, 8), (0, 40)])
def test_rows_are_padded_to_whole_stages_with_zero_columns(dtype, n, D):
    X = torch.randn(n, D).to(dtype)
    R = rows16_operand(X)
    assert R.dtype == dtype and tuple(R.shape) == (n, D) and torch.equal(R, X)
    if n == 0:
        return
    ld = R.stride(0)
    assert ld % 64 == 0 and ld >= D and ld - D < 64 and R.stride(1) == 1 and R.data_ptr() % 16 == 0
    if D % 64:          # copied: the block behind the view is zero beyond D
        assert R.data_ptr() != X.data_ptr()
        block = torch.as_strided(R, (n, ld), (ld, 1))
        assert torch.equal(block[:, :D], X) and float(block[:, D:].float().abs().max()) == 0.0


@pytest.mark.parametrize("dtype", B16_DTYPES)
def test_a_conforming_tensor_is_adopted_and_every_other_one_copied(dtype):
    X = torch.randn(6, 128).to(dtype)
    assert rows16_operand(X).data_ptr() == X.data_ptr()
    wide = torch.randn(6, 256).to(dtype)
    view = wide[:, :128]                     # stride 256 > D: what lies between the rows is not known to be zero
    R = rows16_operand(view)
    assert R.data_ptr() != view.data_ptr() and R.stride(0) == 128 and torch.equal(R, view)
    T = torch.randn(128, 6).to(dtype).t()    # not row-major
    R = rows16_operand(T)
    assert R.stride(1) == 1 and R.stride(0) == 128 and torch.equal(R, T)
    off = torch.randn(6 * 128 + 1).to(dtype)[1:].view(6, 128)          # base 2 bytes off a 16-byte boundary
    assert off.data_ptr() % 16 != 0
    R = rows16_operand(off)
    assert R.data_ptr() % 16 == 0 and torch.equal(R, off)
    with pytest.raises(ValueError):
        rows16_operand(torch.randn(4, 4))


def test_the_switch_is_a_class_attribute_off_by_default_and_no_option():
    from odx import options
    assert HipBackend.native16 is False
    assert "native16" not in getattr(options.Options, "__dataclass_fields__", {}) and not hasattr(options.Options, "native16")


def test_a_features_object_tells_16bit_rows_from_f32_ones():
    F = Features(rows16_operand(torch.randn(4, 70).to(torch.bfloat16)), torch.zeros(4), 70)
    assert F.b16 and F.ld == 128 and F.P is None and F.meta is None and F.f32 is None
    assert not Features(torch.randn(4, 8), torch.zeros(4), 8).b16


@pytest.mark.parametrize("dtype", B16_DTYPES)
def test_a_model_with_16bit_centres_survives_the_model_files(tmp_path, dtype):
    """save_models / load_models keep ny_points_ in its 16-bit type (half the bytes), and the loaded model predicts what the
    saved one did, on the CPU backend."""
    from odx.falkon import GaussianKernel, InCoreFalkon
    rng = np.random.default_rng(0)
    est = InCoreFalkon(kernel=GaussianKernel(6.0), penalty=1e-4, M=40)
    est.ny_points_ = torch.from_numpy(rng.standard_normal((40, 24)).astype(np.float32)).to(dtype)
    est.alpha_ = torch.from_numpy(rng.standard_normal((40, 1)))
    X = torch.from_numpy(rng.standard_normal((9, 24)).astype(np.float32)).to(dtype)
    odx.set_backend(OracleBackend(np.float64))
    try:
        before = est.predict(X)
        storage.save_models(str(tmp_path), "detector", classifier=[est, None])
        clf, _, _ = storage.load_models(str(tmp_path), "detector")
        assert clf[1] is None and clf[0].ny_points_.dtype == dtype and torch.equal(clf[0].ny_points_, est.ny_points_)
        assert torch.equal(clf[0].predict(X), before)
        import os
        small = os.path.getsize(os.path.join(str(tmp_path), "classifier_detector"))
        est.ny_points_ = est.ny_points_.float()
        storage.save_models(str(tmp_path), "rpn", classifier=[est, None])
        # (the archive aligns every tensor's bytes to 64: the saving is the centres' 2 bytes per entry up to that padding)
        assert abs(os.path.getsize(os.path.join(str(tmp_path), "classifier_rpn")) - small - 40 * 24 * 2) <= 64
    finally:
        odx.set_backend(None)
