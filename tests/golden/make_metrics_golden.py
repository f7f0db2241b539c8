"""Mint tests/golden/exit_metrics_ref.npz: the evaluation report's fixture, scored by the reference's OWN metric functions.  Runs only where the
reference tree and its dependencies (scipy, scikit-learn, pandas) are installed; the tests read the .npz and never this script.

    python tests/golden/make_metrics_golden.py <path of the reference's EE directory>

``EE/metrics.py`` is imported by path at mint time -- nothing of its text is stored here.  It imports the ``evaluate`` library at module level
(only ``ece_logits`` uses it, for a remote metric that is in neither tree): an empty stub module of that name stands in.  Called:
``accuracy, brier_loss, nll, f1_micro, f1_macro, aurc_logits``, each as ``metric(references, logits)`` the way ``evaluate_checkpoint``
(EE/eval.py:175-181) calls them -- except ``nll``, which is fed softmax probabilities: on raw logits the reference's ``nll`` hands values above
1 to ``sklearn.metrics.log_loss``, which current scikit-learn refuses.  ECE is not minted.

The reference sorts confidences with an unstable argsort and its AURC depends on the order inside a tie, and two of its functions guess from
``isclose(sum(x), N)`` what their input is: the script asserts that the input has no ties and trips neither guess.
"""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("MMEE_REFERENCE_EE", "")
NAMES = ("accuracy", "brier_loss", "nll", "f1_micro", "f1_macro", "aurc")


def reference_metrics():
    if not os.path.isfile(os.path.join(REF, "metrics.py")):
        raise SystemExit("give the path of the reference's EE directory (argument, or MMEE_REFERENCE_EE)")
    sys.modules.setdefault("evaluate", types.ModuleType("evaluate"))
    spec = importlib.util.spec_from_file_location("ee_reference_metrics", os.path.join(REF, "metrics.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def inputs(seed=515, E1=3, N=1000, K=16):
    """Seeded logits (E1,N,K), float32-representable, and labels (N,): later exits are sharper and more often right.  The labels use classes
    0 .. K-3 only; class K-1 is never predicted either (its logit is pushed down), class K-2 is predicted now and then."""
    rng = np.random.default_rng(seed)
    refs = rng.integers(0, K - 2, N).astype(np.int64)
    L = rng.standard_normal((E1, N, K)) * np.linspace(1.0, 2.5, E1)[:, None, None]
    L[:, np.arange(N), refs] += np.linspace(0.8, 3.0, E1)[:, None]
    L[:, :, K - 1] -= 40.0
    return L.astype(np.float32), refs


def softmax(z):
    z = z - z.max(-1, keepdims=True)
    e = np.exp(z)
    return e / e.sum(-1, keepdims=True)


def check_row(z, refs, what):
    N = z.shape[0]
    srt = np.sort(z, axis=-1)
    assert (srt[:, -1] > srt[:, -2]).all(), f"{what}: a row of logits has two equal maxima"
    conf = softmax(z).max(-1)
    assert len(np.unique(conf)) == N, f"{what}: two documents share a confidence"
    assert not np.isclose(np.sum(z), N), f"{what}: the logits sum to N, the reference would take them for probabilities"
    assert not np.isclose(np.sum(refs), N), f"{what}: the labels sum to N, the reference would take them for correctness"


def score(M, z, refs):
    p = softmax(z)
    return [float(M.accuracy(refs, z)), float(M.brier_loss(refs, z)), float(M.nll(refs, p)), float(M.f1_micro(refs, z)),
            float(M.f1_macro(refs, z)), float(M.aurc_logits(refs, z))]


def main():
    M = reference_metrics()
    L32, refs = inputs()
    L = L32.astype(np.float64)
    E1, N, K = L.shape
    exits = np.random.default_rng(516).integers(0, E1, N).astype(np.int32)
    assert sorted(set(exits.tolist())) == list(range(E1))
    picked = L[exits, np.arange(N)]
    per_exit = []
    for e in range(E1):
        check_row(L[e], refs, f"exit {e}")
        per_exit.append(score(M, L[e], refs))
    check_row(picked, refs, "operating point")
    point = score(M, picked, refs)
    per_exit = np.array(per_exit, dtype=np.float64)
    assert (np.diff(per_exit[:, 0]) > 0).all(), "later exits are more often right"
    absent = [sorted(set(range(K)) - set(refs.tolist()) - set(L[e].argmax(-1).tolist())) for e in range(E1)]
    assert any(absent), "no class is absent from both the references and the predictions of an exit"
    out = os.path.join(HERE, "exit_metrics_ref.npz")
    np.savez_compressed(out, logits=L32, references=refs, exits=exits, names=np.array(NAMES), per_exit=per_exit,
                        point=np.array(point, dtype=np.float64))
    print(f"wrote {out}: {os.path.getsize(out)} bytes; accuracy per exit {per_exit[:, 0].tolist()}, absent classes per exit {absent}")


if __name__ == "__main__":
    main()
