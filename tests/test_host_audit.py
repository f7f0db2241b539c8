"""CPU checks of audited exits (include/mmee.h, behind the cascades): the numpy mask against ``ee_audit_selected``, properties of the hash and
of the restatement tests/audit_ref.py -- the oracle of tests/test_gpu_audit.py --, the reading side (``audit.sample`` / ``audit.consistency``)
on host tensors, the C-ABI's declarations and the refusals that need no device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from . import audit_ref as A
from . import exit_stage_ref as R
from .conftest import ROOT

NEW_SYMBOLS = ("ee_set_audit", "ee_has_audit", "ee_audit_selected", "ee_debug_exit_audit")
SEEDS = (0, 1, 2, 3, 12345)
FRACTIONS = (0.0, 2.0 ** -32, 0.01, 0.25, 0.5, 1.0)


def test_numpy_mask_is_ee_audit_selected(pkg):
    lib = pkg.capi.load()
    for seed in SEEDS:
        for f in FRACTIONS:
            cut = pkg.capi.audit_cut(f)
            assert cut == A.cut_of(f)
            got = np.array([lib.ee_audit_selected(cut, seed, s) for s in range(4096)], bool)
            assert np.array_equal(got, A.mask(4096, f, seed)), (seed, f)
            assert np.array_equal(got, pkg.EarlyExitEngine.audit_mask(4096, f, seed)), (seed, f)
    # slots near 2^31 and a slot base: the product wraps mod 2^32 on both sides
    for slot in (2 ** 31 - 1, 2 ** 31 - 4096, 123456789):
        for seed in (0, 0xFFFFFFFF, 0x80000000):
            assert bool(lib.ee_audit_selected(1 << 31, seed, slot)) == bool(A.selected(1 << 31, seed, slot)), (slot, seed)
    assert np.array_equal(pkg.EarlyExitEngine.audit_mask(50, 0.5, 7, slot_base=2 ** 31 - 60), A.mask(50, 0.5, 7, slot_base=2 ** 31 - 60))


def test_fraction_one_selects_all_zero_none_and_slot_zero_of_seed_zero_always():
    for seed in SEEDS:
        assert A.mask(4096, 1.0, seed).all() and not A.mask(4096, 0.0, seed).any()
    assert A.cut_of(1.0) == 1 << 32 and A.cut_of(0.0) == 0 and A.cut_of(2.0 ** -32) == 1
    assert int(A.hash32(0, 0)) == 0 and A.mask(1, 2.0 ** -32, 0)[0]               # the header says so: callers vary the seed
    assert A.mask(4096, 2.0 ** -32, 0).sum() == 1


def test_slicing_invariance():
    for seed in SEEDS:
        assert np.array_equal(A.mask(64, 0.25, seed)[16:], A.mask(48, 0.25, seed, slot_base=16))
        m = A.mask(4096, 0.25, seed)
        assert np.array_equal(np.concatenate([A.mask(1000, 0.25, seed), A.mask(3096, 0.25, seed, slot_base=1000)]), m)
    # a lower fraction selects a subset under the same seed
    assert (A.mask(4096, 0.25, 3) | ~A.mask(4096, 0.05, 3)).all()


def test_selected_count_is_binomial_within_five_standard_deviations():
    """B = 4096, p = 0.25: mean 1024, standard deviation sqrt(4096 * 0.25 * 0.75) = 27.7; five of them are 139."""
    counts = [int(A.mask(4096, 0.25, seed).sum()) for seed in range(4)]
    assert all(abs(c - 1024) <= 139 for c in counts), counts
    assert counts == [1042, 987, 963, 1012]                                       # the hash as the header defines it
    assert int(A.mask(64, 0.25, 1).sum()) == 17                                   # the forward tests' sample


@pytest.mark.parametrize("n", [1, 63, 65, 1025])
def test_restatement_invariants_on_random_stages(n):
    """Three exits chained on one stage under random decisions: the results are written exactly once per document and where the decision
    without the audit writes them, unselected documents behave as without it, delivered ones stay to the end."""
    rng = np.random.default_rng(n)
    B = n + 11
    cut, seed, base = A.cut_of(0.4), 5, 3
    stage = R.make_stage(n, B, seed=n)
    orig0 = stage["doc_orig"].copy()
    sel = A.selected(cut, seed, np.arange(B) + base)
    delivered = np.full(B, 0x5A5A, np.int64)                                      # dirty: exit 0 must not read it
    plain_exit = np.full(B, -1)                                                   # the same decisions without the audit
    alive_plain = np.zeros(B, bool)
    alive_plain[orig0] = True
    exits, writes_seen = np.full(B, -1), np.zeros(B, int)
    E1 = 4
    sizes = []
    for e in range(E1):
        final = e == E1 - 1
        decision = np.ones(B, bool) if final else rng.random(B) < 0.35            # by original slot: the same for both runs
        o = stage["doc_orig"]
        sizes.append(stage["n"])
        r = A.audit_decide(stage, decision[o], delivered, cut=cut, seed=seed, slot_base=base, exit_index=e, is_final=final)
        gone = alive_plain & decision
        plain_exit[gone & (plain_exit < 0)] = e
        alive_plain &= ~decision
        exits[o[r["writes"]]] = e
        writes_seen[o[r["writes"]]] += 1
        # untouched outside the stage; 0 / 1 inside it after exit 0
        outside = np.ones(B, bool)
        outside[o] = False
        assert np.array_equal(r["delivered"][outside], np.asarray(delivered)[outside])
        if e == 0:
            assert set(np.unique(r["delivered"][o])) <= {0, 1}
        assert not (r["delivered"][o][~sel[o]] == 1).any()                        # only selected documents are ever marked
        kept = o[r["keep"]]
        assert np.array_equal(r["next"]["n_doc_orig"][:r["next"]["n"]], kept)     # stable compaction of the stayers
        assert final or set(o[(r["delivered"][o] == 1)]) <= set(kept)             # a delivered document stays
        assert not final or r["next"]["n"] == 0
        delivered = r["delivered"]
        stage = R.as_stage(r["next"])
    assert (writes_seen[orig0] == 1).all() and np.array_equal(exits[orig0], plain_exit[orig0])
    assert sizes == A.active_at_exit(plain_exit[orig0], sel[orig0], E1)


def test_active_at_exit():
    exits = np.array([0, 0, 1, 2, 3, 3])
    audited = np.array([1, 0, 1, 0, 1, 0], bool)
    assert A.active_at_exit(exits, audited, 4) == [6, 4 + 1, 3 + 2, 2 + 2]
    assert A.active_at_exit(exits, np.ones(6, bool), 4) == [6, 6, 6, 6]
    assert A.active_at_exit(exits, np.zeros(6, bool), 4) == [6, 4, 3, 2]


def test_sample_and_consistency_on_host_tensors(pkg):
    import torch
    rng = np.random.default_rng(4)
    E1, B, K = 5, 200, 6
    al = rng.standard_normal((E1, B, K)).astype(np.float32)
    al[1, ::7] = al[4, ::7]                                                       # some early rows agree with the final one by construction
    al[2, 5, :] = 0.25                                                            # an all-tie row: label 0
    al[4, 9, 1] = al[4, 9, 3] = 9.0                                               # a tie for the final maximum: the lower label
    ex = rng.integers(0, E1, B).astype(np.int32)
    ex[5], ex[9] = 2, 1
    al[1, 9, :] = -1.0
    al[1, 9, 1] = 2.0
    m = A.mask(B, 0.4, 2)
    m[[5, 9]] = True
    ac = rng.random((E1, B)).astype(np.float32)
    out = pkg.EngineOutput(torch.from_numpy(al[ex, np.arange(B)]), torch.from_numpy(ex), torch.from_numpy(ac[ex, np.arange(B)]),
                           all_logits=torch.from_numpy(al), all_crit=torch.from_numpy(ac), audit_mask=torch.from_numpy(m))
    s = pkg.audit.sample(out)
    idx = np.nonzero(m)[0]
    assert np.array_equal(s.index.numpy(), idx) and np.array_equal(s.logits.numpy(), al[:, idx]) and np.array_equal(s.crit.numpy(), ac[:, idx])
    assert np.array_equal(s.exit_layer.numpy(), ex[idx]) and s.num_samples == len(idx)
    am = lambda z: np.argmax(z, -1)                                               # numpy: the first maximum
    d = np.array([(ex[idx] == e).sum() for e in range(E1 - 1)])
    a = np.array([((ex[idx] == e) & (am(al[ex[idx], idx]) == am(al[E1 - 1, idx]))).sum() for e in range(E1 - 1)])
    for rep in (pkg.audit.consistency(out), pkg.audit.consistency(s)):
        assert np.array_equal(rep.delivered, d) and np.array_equal(rep.agree, a) and rep.num_samples == len(idx)
        assert rep.pooled_delivered == d.sum() and rep.pooled_agree == a.sum() and rep.pooled_rate == a.sum() / d.sum()
        assert np.array_equal(rep.rate[d > 0], (a / np.maximum(d, 1))[d > 0]) and np.isnan(rep.rate[d == 0]).all()
    assert a.sum() > 0 and (a < d).any()
    assert np.array_equal(s.references().numpy(), am(al[E1 - 1, idx]))
    two = pkg.AuditSample.concat([s, s])
    assert two.num_samples == 2 * len(idx) and np.array_equal(two.logits.numpy(), np.concatenate([al[:, idx]] * 2, 1))
    assert pkg.audit.consistency(two).pooled_agree == 2 * a.sum()
    with pytest.raises(ValueError, match="not audited"):
        pkg.audit.sample(pkg.EngineOutput(out.logits, out.exit_layer, out.confidence, all_logits=out.all_logits, all_crit=out.all_crit))
    with pytest.raises(ValueError, match="want_all"):
        pkg.audit.sample(pkg.EngineOutput(out.logits, out.exit_layer, out.confidence, audit_mask=out.audit_mask))
    with pytest.raises(ValueError, match="no samples"):
        pkg.AuditSample.concat([])


def test_the_c_abi_declares_the_new_entry_points_and_the_binding_knows_them(pkg):
    header = open(os.path.join(ROOT, "include", "mmee.h")).read()
    declared = set(re.findall(r"^\w[\w\s\*]*?\b(ee_\w+)\s*\(", header, flags=re.M))
    lib = pkg.capi.load()
    for name in NEW_SYMBOLS:
        assert name in declared and name in pkg.capi.SYMBOLS and hasattr(lib, name), name
    assert int(re.search(r"#define\s+MMEE_ABI_VERSION\s+(\d+)", header).group(1)) == pkg.capi.ABI_VERSION == 4      # four functions: no struct changed
    flat = re.sub(r"\s+", " ", re.sub(r"\n \*", " ", header))                      # the comment's line prefix goes, the hash's `*=` stays
    # the header states the definition once: the constants in their order, the always-selected slot, the refusals and what is not built
    for words in ("0x9E3779B1u ^ seed", "x ^= x >> 16; x *= 0x85EBCA6Bu; x ^= x >> 13; x *= 0xC2B2AE35u; x ^= x >> 16;",
                  "(seed 0, slot 0) hashes to 0 and is selected under every cut > 0: callers vary the seed per call",
                  "floor(fraction 2^32 + 0.5)", "Not built: audit under quotas, with the result stream, in captured graphs, on cascade stages; a per-exit share; "
                  "a selection that depends on content; a confidence bound on the agreement rate"):
        assert words in flat, words
    assert C.sizeof(pkg.capi.DebugExitAuditArgs) == C.sizeof(pkg.capi.DebugExitDecideArgs) + 8 + 4 + 4 + C.sizeof(C.c_void_p)
    # one definition of the test: the kernels' header has it, the C-ABI's translation unit calls it
    csrc = os.path.join(ROOT, "multi-modal-early-exit_amd", "csrc")
    assert "__host__ __device__ inline bool audit_selected(" in open(os.path.join(csrc, "mmee_kernels.h")).read()
    assert "return audit_selected(cut, seed, slot)" in open(os.path.join(csrc, "capi_query.hip")).read()
    assert open(os.path.join(csrc, "exit_stage.hip")).read().count("0x9E3779B1") == 0


def test_refusals_that_need_no_device(pkg):
    lib = pkg.capi.load()
    args = pkg.capi.DebugExitAuditArgs()
    assert lib.ee_debug_exit_audit(None, None) != 0 and "args must not be NULL" in pkg.capi.last_error()
    args.cut, args.decide.no_exit = 1, 1
    assert lib.ee_debug_exit_audit(C.byref(args), None) != 0 and "no_exit must be 0" in pkg.capi.last_error()
    args.decide.no_exit, args.cut = 0, 0
    assert lib.ee_debug_exit_audit(C.byref(args), None) != 0 and "cut 0 outside [1, 2^32]" in pkg.capi.last_error()
    args.cut = (1 << 32) + 1
    assert lib.ee_debug_exit_audit(C.byref(args), None) != 0 and "outside [1, 2^32]" in pkg.capi.last_error()
    args.cut, args.slot_base = 1 << 32, -1
    assert lib.ee_debug_exit_audit(C.byref(args), None) != 0 and "slot_base -1 is negative" in pkg.capi.last_error()
    args.slot_base = 0
    assert lib.ee_debug_exit_audit(C.byref(args), None) != 0 and "delivered must not be NULL" in pkg.capi.last_error()
    assert lib.ee_set_audit(None, 1, 0, 0) != 0 and lib.ee_has_audit(None) == 0
    for bad in (-0.01, 1.0000001, float("nan")):
        with pytest.raises(ValueError, match="outside"):
            pkg.capi.audit_cut(bad)
        with pytest.raises(ValueError, match="outside"):
            pkg.EarlyExitEngine.audit_mask(8, bad, 0)
