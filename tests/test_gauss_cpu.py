"""Novelty scores without a GPU: include/ivit_gauss.h declares four entries under version 1 and the binding follows it; the fit and the
numpy statement against the Mahalanobis distance computed directly; the leading-subspace form; an empty class; the LDA head."""
import re

import numpy as np
import pytest

import ivit_amd as iv
from ivit_amd import _abi, _lib, gauss
from ivit_amd.predict import gauss_fit_reference, gauss_score_reference, probe_stats_reference

ENTRIES = {"ivit_gauss_model_bytes": 4, "ivit_gauss_prepare": 10, "ivit_gauss_workspace_bytes": 6, "ivit_gauss_score": 15}


def test_gauss_header_declares_entries_under_version_1_bound_and_exported():
    hdr = open(_abi.GAUSS_HEADER).read()
    assert re.search(r'#include "ivit\.h"', hdr)
    assert _abi.GAUSS_ABI.constants == {"IVIT_GAUSS_VERSION": 1} and _lib.IVIT_GAUSS_VERSION == 1
    assert list(_abi.GAUSS_ABI.functions) == list(ENTRIES) == list(_lib.GAUSS_SIGNATURES) == list(_lib.GAUSS_RESTYPES)
    for name in ENTRIES:                                  # one "Alignment:" and one "Overlap:" line in front of every entry
        m = re.search(r"\bint %s\(" % name, hdr)
        front = hdr[hdr.rfind(";", 0, m.start()) + 1:m.start()]
        assert len(re.findall(r"\bAlignment:", front)) == 1 and len(re.findall(r"\bOverlap:", front)) == 1, name
    iv.build()
    lib = _lib.load()
    for name, nparams in ENTRIES.items():                 # every bound name is exported, with the header's parameter count
        bound = getattr(lib, name)
        assert len(_lib.GAUSS_SIGNATURES[name]) == nparams and bound.argtypes == _lib.GAUSS_SIGNATURES[name] and bound.restype is _lib._I
    assert "ivit_gauss.h" in _lib.SOURCES


@pytest.fixture(scope="module")
def five():
    """five classes of int8 rows, dim 64, a within-class covariance of condition number <= 100 (standard deviations 5 .. 30 along a
    random orthogonal basis); x, labels, the class means and the pooled covariance computed directly from the rows"""
    rng = np.random.default_rng(0)
    basis = np.linalg.qr(rng.normal(size=(64, 64)))[0]
    lab = rng.integers(5, size=4000)
    pts = rng.normal(size=(5, 64)) * 15.0
    x = np.clip(np.rint(pts[lab] + (rng.normal(size=(4000, 64)) * np.geomspace(5.0, 30.0, 64)) @ basis.T), -128, 127).astype(np.int8)
    xf = x.astype(np.float64)
    mu = np.stack([xf[lab == c].mean(axis=0) for c in range(5)])
    cov = sum((xf[lab == c] - mu[c]).T @ (xf[lab == c] - mu[c]) for c in range(5)) / (4000 - 5)
    assert np.linalg.cond(cov) <= 100
    return x, lab, mu, cov


def direct(x, mu, metric):
    d = x.astype(np.float64)[:, None, :] - mu[None]
    return np.einsum("ncd,de,nce->nc", d, metric, d)


@pytest.mark.parametrize("rank", [None, 32])
def test_fit_and_reference_equal_the_direct_mahalanobis_distance(five, rank):
    x, lab, mu, cov = five
    model = gauss_fit_reference(*probe_stats_reference(x, lab, 5), shrinkage=0, rank=rank)
    assert model[0].shape == (rank or 64, 64) and all(a.dtype == np.float64 for a in model)
    lam, U = np.linalg.eigh(cov)
    keep = np.argsort(lam)[::-1][:rank or 64]             # the projector onto the leading eigenvectors, inside the inverse
    want = direct(x, mu, (U[:, keep] / lam[keep]) @ U[:, keep].T)
    dist, cls, q, best = gauss_score_reference(x, *model)
    assert np.allclose(dist, want.min(axis=1), rtol=1e-9, atol=0) and np.array_equal(cls, want.argmin(axis=1))
    assert cls.dtype == np.int32 and np.array_equal(dist, q - best)


def test_an_empty_class_is_never_chosen_and_all_empty_gives_infinity(five):
    x, lab, _, _ = five
    Wh, t, Wc, bc = gauss_fit_reference(*probe_stats_reference(x, np.where(lab == 2, -1, lab), 5))
    assert bc[2] == -np.inf and not Wc[2].any() and np.isfinite(np.delete(bc, 2)).all()
    dist, cls, q, best = gauss_score_reference(x, Wh, t, Wc, bc)
    assert (cls != 2).all() and np.isfinite(dist).all()
    dist, cls, q, best = gauss_score_reference(x[:3], Wh, t, Wc, np.full(5, -np.inf))
    assert (cls == 0).all() and (best == -np.inf).all() and (dist == np.inf).all() and np.isfinite(q).all()
    with pytest.raises(ValueError):
        gauss.GaussModel(Wh, t, Wc, bc).head(0.05)


def test_head_reproduces_cls_and_the_model_survives_a_file(five, tmp_path):
    x, lab, _, _ = five
    model = gauss.fit(probe_stats_reference(x, lab, 5))
    assert (model.R, model.dim, model.C) == (64, 64, 5) and model.Wh.dtype == np.float32
    cls = gauss_score_reference(x, model.Wh, model.t, model.Wc, model.bc)[1]
    assert (model.head(0.05).logits_reference(x).argmax(axis=1) == cls).mean() >= 0.99 and (cls == lab).mean() > 0.9
    model.save(tmp_path / "m.npz")
    back = gauss.GaussModel.load(tmp_path / "m.npz")
    assert all(np.array_equal(getattr(back, n), getattr(model, n)) for n in ("Wh", "t", "Wc", "bc"))
    assert gauss.auroc([1, 2, 3], [3, 4]) == pytest.approx(11 / 12) and gauss.fpr_at_tpr(np.arange(100), [10, 94, 95, 200]) == 0.5
