"""The factor risk model's two C entries (include/fmx.h: fmx_risk_books, fmx_risk_mvo_books)
called through ctypes with raw device pointers, as a C caller would: K = 1 factor, A = 3 assets,
small enough to check by hand."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _lib():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import factormodeling_amd._lib as L
    return L, L.load(), torch


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def test_risk_books_and_risk_mvo_books_through_the_c_abi():
    L, lib, torch = _lib()
    dev = "cuda"
    B = torch.tensor([[[1.0, 2.0, -1.0]]], dtype=torch.float64, device=dev)          # [K=1][D=1][A=3]
    Fc = torch.tensor([[[4e-4]]], dtype=torch.float64, device=dev)
    S2 = torch.tensor([[1e-4, 2e-4, 3e-4]], dtype=torch.float64, device=dev)
    W = torch.tensor([[[0.5, 0.5, -1.0]]], dtype=torch.float64, device=dev)
    var = torch.empty((1, 1, 3), dtype=torch.float64, device=dev)
    expo, contrib = torch.empty((1, 1, 1), dtype=torch.float64, device=dev), torch.empty((1, 1, 1), dtype=torch.float64, device=dev)
    marg = torch.empty((1, 1, 3), dtype=torch.float64, device=dev)
    stream = L.stream_ptr()
    assert lib.fmx_risk_books(_p(B), _p(Fc), _p(S2), _p(W), None, None, 1, 1, 3, 1, _p(var), _p(expo), _p(contrib),
                              _p(marg), stream) == 0
    torch.cuda.synchronize()
    b = 0.5 * 1 + 0.5 * 2 + 1.0
    fvar, svar = b * b * 4e-4, 0.25 * 1e-4 + 0.25 * 2e-4 + 3e-4
    np.testing.assert_allclose(var.cpu().numpy()[0, 0], [fvar + svar, fvar, svar], rtol=1e-14)
    np.testing.assert_allclose(expo.cpu().numpy().ravel(), [b], rtol=1e-15)
    np.testing.assert_allclose(contrib.cpu().numpy().ravel(), [fvar], rtol=1e-14)
    np.testing.assert_allclose(marg.cpu().numpy()[0, 0], np.array([1.0, 2.0, -1.0]) * 4e-4 * b
                               + np.array([1e-4, 2e-4, 3e-4]) * np.array([0.5, 0.5, -1.0]), rtol=1e-14)
    # K outside 1..32 is an argument error
    assert lib.fmx_risk_books(_p(B), _p(Fc), _p(S2), _p(W), None, None, 33, 1, 3, 1, _p(var), _p(expo), _p(contrib),
                              None, stream) == 1  # FMX_ERR_ARG
    assert b"K" in lib.fmx_last_error()

    # the QP: longs {0, 1}, short {2} = -1; w0 + w1 = 1 minimises
    # (w0 + 2 w1 + 1)^2 4e-4 + 1e-4 w0^2 + 2e-4 w1^2: with w1 = 1 - w0, g(w0) = 4e-4 (3 - w0)^2 + 1e-4 w0^2
    # + 2e-4 (1 - w0)^2, g' = 0 at w0 = (24e-4 + 4e-4) / (8e-4 + 2e-4 + 4e-4) = 2 -> the box end w0 = 1
    X = torch.tensor([[1.0, 2.0, -1.0]], dtype=torch.float64, device=dev)
    mrow = torch.tensor([0], dtype=torch.int32, device=dev)
    Wq = torch.empty((1, 3), dtype=torch.float64, device=dev)
    counts = torch.empty((1, 2), dtype=torch.float64, device=dev)
    info = torch.empty((1, 6), dtype=torch.float64, device=dev)
    assert lib.fmx_risk_mvo_books_work_bytes(3, 1, 1) == 0
    assert lib.fmx_risk_mvo_books(_p(B), _p(Fc), _p(S2), 1, 1, 3, _p(mrow), _p(X), None, 1, 1.0, 20000, 1e-9, _p(Wq),
                                  _p(counts), _p(info), stream) == 0
    torch.cuda.synchronize()
    print("w", Wq.cpu().numpy(), "info", info.cpu().numpy())
    assert info.cpu().numpy()[0, 0] == 0 and list(counts.cpu().numpy()[0]) == [2, 1]
    np.testing.assert_allclose(Wq.cpu().numpy()[0], [1.0, 0.0, -1.0], atol=1e-8)
    bad = torch.tensor([1], dtype=torch.int32, device=dev)
    assert lib.fmx_risk_mvo_books(_p(B), _p(Fc), _p(S2), 1, 1, 3, _p(bad), _p(X), None, 1, 1.0, 20000, 1e-9, _p(Wq),
                                  _p(counts), _p(info), stream) == 1
    assert b"model_row" in lib.fmx_last_error()
