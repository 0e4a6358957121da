"""computeWAIC, host side (CPU only): the host path is what it was, the argument builder of the
device path (post._waic_args: shapes, nf padding, covariate-dependent levels, refusals), and the
numpy restatement of the device's shifted sums (tests/waic_oracle.py) against the literal form
of R/computeWAIC.R:124-129 and against mpmath where the literal form overflows."""
import ctypes as C

import mpmath as mp
import numpy as np
import pytest

import waic_oracle as W
from helpers import H
from hmsc_amd import post as P
from test_golden_td import td_model, td_postlist


def _arr(ptr, n, dt=np.float64):
    return np.ctypeslib.as_array(ptr, shape=(n,)).astype(dt)


def test_host_path_is_unchanged_on_td():
    """test-WAIC.R:4 through the new signature: device=None is the host loop, byUnit its pieces."""
    hM = td_model()
    hM.postList = td_postlist(hM)
    w = H.computeWAIC(hM)
    assert round(w, 1) == 0.8
    assert H.computeWAIC(hM, device=None) == w
    u = H.computeWAIC(hM, device=None, byUnit=True)
    assert u["WAIC"] == w and u["Bl"].shape == (hM.ny,) and u["V"].shape == (hM.ny,)
    assert float(np.mean(u["Bl"] + u["V"])) == w


def _two_level_model(seed=3):
    rng = np.random.default_rng(seed)
    ny, ns, nc = 24, 5, 2
    Pi = np.column_stack([np.arange(ny) + 1, rng.permutation(np.arange(ny) % 6) + 1])
    xs = [None, np.column_stack([np.ones(6), rng.standard_normal(6)])]
    hM = W.duck_model(rng.integers(0, 2, (ny, ns)).astype(float), rng.standard_normal((ny, nc)), [2] * ns,
                      Pi=Pi, nps=[ny, 6], xs=xs)
    post = W.random_post(hM, 4, [3, 2], seed, nf_jitter=True)
    hM.postList = [post]
    return hM, post


def test_argument_builder_shapes_padding_and_xdim():
    """Level 0 has nf = 3, 2, 3, 2 over the samples (padded to 3 with zero factors); level 1 is
    covariate-dependent with xDim = 2 and becomes two device levels sharing its Pi column."""
    hM, post = _two_level_model()
    a, keep, dims = P._waic_args(hM, post, ghN=7, device=0, sample_chunk=3)
    ny, ns, nc, S = 24, 5, 2, 4
    assert (a.ny, a.ns, a.nc, a.nr, a.nsamples, a.ghN, a.sample_chunk) == (ny, ns, nc, 3, S, 7, 3)
    assert dims == dict(S=S, nr=3, np=[ny, 6, 6], nf=[3, 2, 2])
    assert _arr(a.np, 3, np.int32).tolist() == [ny, 6, 6] and _arr(a.nf, 3, np.int32).tolist() == [3, 2, 2]
    Pi = _arr(a.Pi, ny * 3, np.int32).reshape(ny, 3, order="F")
    assert (Pi[:, 0] == hM.Pi[:, 0]).all() and (Pi[:, 1] == hM.Pi[:, 1]).all() and (Pi[:, 2] == hM.Pi[:, 1]).all()
    np.testing.assert_array_equal(_arr(a.Y, ny * ns).reshape(ny, ns, order="F"), hM.Y)
    Beta = _arr(a.Beta, S * nc * ns).reshape(S, ns, nc)
    sigma = _arr(a.sigma, S * ns).reshape(S, ns)
    eta0 = _arr(a.Eta[0], S * ny * 3).reshape(S, 3, ny)
    lam0 = _arr(a.Lambda[0], S * 3 * ns).reshape(S, ns, 3)
    x = hM.rL[1].x
    for s, smp in enumerate(post):
        np.testing.assert_array_equal(Beta[s].T, smp["Beta"])
        np.testing.assert_array_equal(sigma[s], smp["sigma"])
        nf = smp["Eta"][0].shape[1]
        assert nf == (2 if s % 2 else 3)
        np.testing.assert_array_equal(eta0[s, :nf].T, smp["Eta"][0])
        np.testing.assert_array_equal(lam0[s, :, :nf].T, smp["Lambda"][0])
        assert (eta0[s, nf:] == 0).all() and (lam0[s, :, nf:] == 0).all()
        for k in range(2):
            ek = _arr(a.Eta[1 + k], S * 6 * 2).reshape(S, 2, 6)[s].T
            lk = _arr(a.Lambda[1 + k], S * 2 * ns).reshape(S, ns, 2)[s].T
            np.testing.assert_array_equal(ek, smp["Eta"][1] * x[:, k:k + 1])
            np.testing.assert_array_equal(lk, smp["Lambda"][1][:, :, k])
    gx, gw = np.polynomial.hermite.hermgauss(7)
    np.testing.assert_array_equal(_arr(a.gx, 7), gx)
    np.testing.assert_array_equal(_arr(a.gw, 7), gw)
    assert not a.Eta[3] and not a.Lambda[3]
    # what the kernel contracts equals the host's linear predictor
    from hmsc_amd.sampler import level_lran
    for s, smp in enumerate(post):
        E = hM.X @ smp["Beta"] + level_lran(smp["Eta"][0], smp["Lambda"][0], hM.Pi[:, 0] - 1) + \
            level_lran(smp["Eta"][1], smp["Lambda"][1], hM.Pi[:, 1] - 1, x)
        Ed = hM.X @ Beta[s].T + eta0[s].T[Pi[:, 0] - 1] @ lam0[s].T
        for k in range(2):
            Ed = Ed + _arr(a.Eta[1 + k], S * 12).reshape(S, 2, 6)[s].T[Pi[:, 1 + k] - 1] @ \
                _arr(a.Lambda[1 + k], S * 2 * ns).reshape(S, ns, 2)[s].T
        np.testing.assert_allclose(Ed, E, rtol=0, atol=1e-13)


def test_refusals_name_their_reason():
    hM, post = _two_level_model()
    with pytest.raises(ValueError, match="nsamples = 1"):
        P._waic_args(hM, post[:1])
    hM.ncRRR = 1
    with pytest.raises(ValueError, match="ncRRR"):
        P._waic_args(hM, post)
    hM.postList = [post]
    with pytest.raises(ValueError, match="ncRRR"):
        H.computeWAIC(hM, device=0)


def test_shifted_sums_equal_the_literal_form():
    """Where exp(val) is finite and non-zero the two forms agree to 1e-13 of max(1, |value|):
    Bl = -log(mean) is conditioned absolutely, not relatively, where the mean is near 1."""
    rng = np.random.default_rng(0)
    for centre, spread in ((-3.0, 1.0), (-400.0, 5.0), (-700.0, 2.0), (0.0, 0.1)):
        val = centre + spread * rng.standard_normal((40, 17))
        Bl0, V0, w0 = W.literal(val)
        Bl1, V1, w1 = W.shifted(val)
        assert np.isfinite(Bl0).all()
        assert (np.abs(Bl1 - Bl0) <= 1e-13 * np.maximum(1.0, np.abs(Bl0))).all()
        assert (np.abs(V1 - V0) <= 1e-13 * np.maximum(1.0, np.abs(V0))).all()
        assert abs(w1 - w0) <= 1e-13 * max(1.0, abs(w0))


def test_shifted_sums_stay_finite_where_the_literal_form_overflows():
    rng = np.random.default_rng(1)
    val = -800.0 + 3.0 * (2 * rng.random((25, 6)) - 1)
    Bl0, _, w0 = W.literal(val)
    assert np.isinf(Bl0).all() and np.isinf(w0)
    Bl, V, w = W.shifted(val)
    assert np.isfinite(Bl).all() and np.isfinite(w)
    for i in range(val.shape[1]):
        rb, rv = W.mp_site(val[:, i])
        assert abs(mp.mpf(float(Bl[i])) - rb) <= 1e-13 * abs(rb)
        assert abs(mp.mpf(float(V[i])) - rv) <= 1e-13 * abs(rv)
