"""The logistic probe without a GPU: include/ivit_logreg.h declares two entries under version 1 and the binding follows it, the numpy
statement against a direct softmax, and fit_logistic's optimiser over the numpy statement on a separable problem."""
import re

import numpy as np

import ivit_amd as iv
from ivit_amd import _abi, _lib
from ivit_amd.predict import logreg_reference
from ivit_amd.probe import fit_logistic

ENTRIES = {"ivit_logreg_workspace_bytes": 5, "ivit_logreg_loss_grad": 16}


def test_logreg_header_declares_entries_under_version_1_bound_and_exported():
    hdr = open(_abi.LOGREG_HEADER).read()
    assert re.search(r'#include "ivit\.h"', hdr)
    assert _abi.LOGREG_ABI.constants == {"IVIT_LOGREG_VERSION": 1} and _lib.IVIT_LOGREG_VERSION == 1
    assert list(_abi.LOGREG_ABI.functions) == list(ENTRIES) == list(_lib.LOGREG_SIGNATURES)
    for name in ENTRIES:                                  # one "Alignment:" and one "Overlap:" line in front of every entry
        m = re.search(r"\bint %s\(" % name, hdr)
        front = hdr[hdr.rfind(";", 0, m.start()) + 1:m.start()]
        assert len(re.findall(r"\bAlignment:", front)) == 1 and len(re.findall(r"\bOverlap:", front)) == 1, name
    iv.build()
    lib = _lib.load()
    for name, nparams in ENTRIES.items():                 # every bound name is exported, with the header's parameter count
        bound = getattr(lib, name)
        assert len(_lib.LOGREG_SIGNATURES[name]) == nparams and bound.argtypes == _lib.LOGREG_SIGNATURES[name] and bound.restype is _lib._I
    assert "ivit_logreg.h" in _lib.SOURCES


def test_reference_against_a_direct_softmax():
    rng = np.random.default_rng(0)
    x, lab = rng.integers(-128, 128, size=(7, 64)).astype(np.int8), np.array([0, 2, 1, 3, -1, 2, 0])      # two rows outside 0 .. 2
    W, b, s = rng.normal(size=(3, 64)) * 0.05, rng.normal(size=3), 0.03
    loss, gW, gb, correct = logreg_reference(x, lab, W, b, s)
    keep = [0, 1, 2, 5, 6]
    z = np.float64(np.float32(s)) * x[keep].astype(np.float64) @ W.T + b
    p = np.exp(z) / np.exp(z).sum(axis=1, keepdims=True)
    g = p - np.eye(3)[lab[keep]]
    assert np.isclose(loss, -np.log(p[np.arange(5), lab[keep]]).sum(), rtol=1e-12)
    assert np.allclose(gW, g.T @ x[keep], rtol=1e-10, atol=1e-10) and np.allclose(gb, g.sum(axis=0), rtol=1e-10, atol=1e-12)
    assert correct.tolist() == [5, int((z.argmax(axis=1) == lab[keep]).sum())] and correct.dtype == np.int64
    z2 = logreg_reference(x[:1], [1], np.ones((3, 64)), np.zeros(3), 1.0)      # equal logits: the smallest index is the argmax
    assert z2[3].tolist() == [1, 0] and np.isclose(z2[0], np.log(3.0))


def test_fit_logistic_over_the_reference_separates_and_converges():
    rng = np.random.default_rng(1)
    lab = rng.integers(3, size=200)
    means = rng.integers(-40, 41, size=(3, 64))
    x = np.clip(means[lab] + rng.integers(-25, 26, size=(200, 64)), -128, 127).astype(np.int8)
    head = fit_logistic(x, lab, 3, 0.02, l2=1e-2, iters=300, tol=1e-6, evaluate=logreg_reference)
    info = head.fit_info
    assert info["train_acc"] == 1.0 and info["n"] == 200 and info["grad_norm"] < 1e-6, info
    assert (head.logits_reference(x).argmax(axis=1) == lab).all()
    loss, gW, gb, _ = logreg_reference(x, lab, head.weight, head.bias, 0.02)   # the gradient at the returned head, restated
    g = np.concatenate([(np.float64(np.float32(0.02)) * gW / 200 + 1e-2 * head.weight).ravel(), gb / 200])
    assert np.linalg.norm(g) < 1e-6
