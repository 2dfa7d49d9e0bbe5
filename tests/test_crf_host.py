"""CPU tests of the dense-CRF feature: known answers of the numpy oracle (tests/crf_oracle.py) that need no GPU, the
unary energies of both the oracle and the package against hand-written values, and the `backend` keyword of do_crf."""
import numpy as np
import pytest

import dl3_amd  # noqa: F401
from dl3_amd import capi
from dl3_amd import crf as C
from dl3_amd import utils as U
from tests import crf_oracle as O


def test_oracle_parameters_are_the_packages():
    assert O.PARAMS == U.CRF_PARAMS
    assert np.array_equal(C.kernel_params(), np.array([3, 3, 3, 80, 13, 10], np.float32))


def test_unary_from_labels_hand_written_case():
    """2 x 3 label map, L = 3, gt_prob 0.7: n_e = -log(0.3 / 2), p_e = -log(0.7), unsure = -log(1 / 3)"""
    labels = np.array([[0, 1, 2], [2, 0, 1]])
    n, p, u = -np.log(0.15), -np.log(0.7), -np.log(1 / 3)
    want_plain = np.array([[p, n, n, n, p, n],
                           [n, p, n, n, n, p],
                           [n, n, p, p, n, n]])
    # zero_unsure: label k >= 1 owns row k - 1, label 0 (columns 0 and 4) is unsure everywhere
    want_unsure = np.array([[u, p, n, n, u, p],
                            [u, n, p, p, u, n],
                            [u, n, n, n, u, n]])
    for fn in (lambda zu: O.unary_from_labels(labels, 3, 0.7, zu), lambda zu: C.unary_from_labels(labels, 3, 0.7, zu)):
        assert np.allclose(fn(False), want_plain, rtol=1e-6, atol=0)
        assert np.allclose(fn(True), want_unsure, rtol=1e-6, atol=0)
    assert C.unary_from_labels(labels, 3, 0.7, True).dtype == np.float32


def test_uniform_image_and_mask_keep_the_labels():
    im = np.full((9, 11, 3), 77, np.uint8)
    labels = np.ones(99, np.int64)
    Q, E, MAP = O.inference(im, O.unary_from_labels(labels, 2, 0.7, False))
    assert np.array_equal(MAP, labels)
    assert np.allclose(Q.sum(0), 1.0, atol=1e-12)


def test_one_disagreeing_pixel_in_a_flat_region_is_overruled():
    im = np.full((12, 12, 3), 120, np.uint8)
    labels = np.zeros((12, 12), np.int64)
    labels[5, 6] = 1
    labels[0, 0] = 1  # keeps np.unique at two labels when run through do_crf
    out, Q, E, MAP, colors = O.do_crf(im, labels, zero_unsure=False)
    assert np.all(out == 0)
    assert np.allclose(Q.sum(0), 1.0, atol=1e-12)


def test_quadrant_image_with_label_noise_is_cleaned():
    rng = np.random.default_rng(3)
    H = W = 24
    y, x = np.mgrid[:H, :W]
    region = (2 * (y >= H // 2) + (x >= W // 2)).astype(np.int64)
    palette = np.array([[200, 30, 30], [30, 200, 30], [30, 30, 200], [220, 220, 40]])
    im = np.clip(palette[region] + rng.integers(-5, 6, (H, W, 3)), 0, 255).astype(np.uint8)
    mask = region.copy()
    flip = rng.random((H, W)) < 0.25
    mask[flip] = rng.integers(0, 4, int(flip.sum()))
    out, Q, _, _, _ = O.do_crf(im, mask, zero_unsure=False)
    assert (out != region).sum() < (mask != region).sum()
    assert np.allclose(Q.sum(0), 1.0, atol=1e-12)


def test_brute_force_gaussian_message_equals_the_separable_evaluation():
    rng = np.random.default_rng(4)
    H, W, L = 13, 17, 3
    Q = rng.random((H * W, L))
    brute = O.message(O.gauss_features(H, W, (3, 3)), Q)
    kx = np.exp(-0.5 * ((np.arange(W)[:, None] - np.arange(W)[None, :]) / 3.0) ** 2)
    ky = np.exp(-0.5 * ((np.arange(H)[:, None] - np.arange(H)[None, :]) / 3.0) ** 2)
    sep = np.einsum("ya,xb,abl->yxl", ky, kx, Q.reshape(H, W, L)).reshape(H * W, L)
    assert np.abs(brute - sep).max() <= 1e-12 * np.abs(sep).max()


def test_do_crf_backend_keyword():
    im, mask = np.zeros((8, 8, 3), np.uint8), np.arange(64).reshape(8, 8) % 2
    with pytest.raises(ValueError, match="backend"):
        U.do_crf(im, mask, backend="lattice")
    try:
        import pydensecrf  # noqa: F401
    except ImportError:
        with pytest.raises(ImportError, match="pydensecrf"):  # the default path is the reference's
            U.do_crf(im, mask, backend="pydensecrf")
    # a single-valued mask has no CRF to run (pydensecrf's unary divides by n_labels - 1): returned as it is
    one = np.full((8, 8), 5)
    assert np.array_equal(U.do_crf(im, one, backend="device"), one)


def test_device_backend_fails_loudly_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    im, mask = np.zeros((8, 8, 3), np.uint8), np.arange(64).reshape(8, 8) % 2
    with pytest.raises(capi.DL3Error):
        U.do_crf(im, mask, backend="device")
    with pytest.raises(capi.DL3Error):
        C.dense_crf(im[None], mask[None])
