"""GPU parity: the HIP path (through the C-ABI) against the committed golden vectors and the oracle.

Tolerances (north star): logits within 1e-4 abs of the reference CPU path, exit indices bit-exact.
"""
import numpy as np
import pytest

from .conftest import BASE_EE, MATRIX_CASES, MATRIX_SEEDS, TINY_CASES, load_golden, matrix_config, report_measured

pytestmark = pytest.mark.gpu

LOGIT_TOL = 1e-4
# Engines of this suite are built with xprobe=False: the engine's default probe (round 4: the X-space CLS probe wherever the library has it)
# matches whole layers to tolerance only, and many tests here assert BIT identity between schedules / with the dump-all rows.  The X-space
# probe is asked for explicitly where it is the subject (test_xspace_probe_*, the config-1 sweep, the config-2 32-document test,
# test_engine_default_is_the_xspace_probe).


def _engine(pkg, cfg, W, max_docs, T, precision="fp32"):
    eng = pkg.EarlyExitEngine(cfg, max_docs=max_docs, max_text_len=T, precision=precision, xprobe=False)
    eng.load_weights(W)
    return eng


def _np(t):
    return None if t is None else t.detach().cpu().numpy()


@pytest.mark.parametrize("name", list(TINY_CASES))
@pytest.mark.parametrize("dense_rows", [False, True])
def test_tiny_dump_all_matches_golden(pkg, name, dense_rows):
    g = load_golden(name)
    cfg = pkg.ModelConfig.tiny(EE_config=TINY_CASES[name])
    W = pkg.synth.make_weights(cfg, seed=int(g["seed_w"]))
    docs = {k[3:]: v for k, v in g.items() if k.startswith("in_")}
    eng = _engine(pkg, cfg, W, max_docs=8, T=int(g["text_len"]))
    out = eng.forward(docs["input_ids"], docs["attention_mask"], docs["bbox"], docs["pixel_values"], dump_all=True,
                      dense_rows=dense_rows, want_all=True, want_head=True, want_hidden_cls=True, validate=True)
    np.testing.assert_allclose(_np(out.hidden_cls), g["hidden_cls"], rtol=0, atol=5e-5)
    np.testing.assert_allclose(_np(out.head_logits), g["exit_logits"], rtol=0, atol=LOGIT_TOL)
    np.testing.assert_allclose(_np(out.head_crit), g["exit_crit"], rtol=0, atol=2e-5)
    np.testing.assert_allclose(_np(out.all_logits), g["logits_store"], rtol=0, atol=LOGIT_TOL)
    np.testing.assert_allclose(_np(out.logits), g["logits"], rtol=0, atol=LOGIT_TOL)
    E = g["exit_logits"].shape[0]
    assert (_np(out.exit_layer) == E).all()
    eng.close()


def _margin_ok(store, thr, margin=1e-3):
    e = np.exp(store - store.max(-1, keepdims=True))
    conf = (e / e.sum(-1, keepdims=True)).max(-1)
    return np.abs(conf - thr).min() > margin


@pytest.mark.parametrize("dense_rows", [False, True])
def test_tiny_early_exit_matches_reference_policy(pkg, oracle, dense_rows):
    g = load_golden("tiny_ramp")
    cfg = pkg.ModelConfig.tiny(EE_config=TINY_CASES["tiny_ramp"])
    W = pkg.synth.make_weights(cfg, seed=int(g["seed_w"]))
    docs = {k[3:]: v for k, v in g.items() if k.startswith("in_")}
    eng = _engine(pkg, cfg, W, max_docs=8, T=int(g["text_len"]))
    for i in range(4):
        thr = float(g[f"pol_thr{i}"])
        assert _margin_ok(g["logits_store"], thr, 1e-5) or thr == 0.0 or thr > 1.0
        out = eng.forward(docs["input_ids"], docs["attention_mask"], docs["bbox"], docs["pixel_values"], thresholds=thr,
                          dense_rows=dense_rows, want_all=True)
        ex = _np(out.exit_layer)
        assert np.array_equal(ex, g[f"pol_exits{i}"]), (thr, ex, g[f"pol_exits{i}"])
        np.testing.assert_allclose(_np(out.logits), g[f"pol_pred{i}"], rtol=0, atol=LOGIT_TOL)
        counts = eng.stage_counts()
        # documents entering stage e = documents that did not leave through an earlier exit
        surv = [int((g[f"pol_exits{i}"] >= e).sum()) for e in range(len(counts["docs"]))]
        assert counts["docs"] == surv
        # exits that a document never reached stay NaN; reached ones match the store
        al = _np(out.all_logits)
        for n in range(al.shape[1]):
            for e in range(al.shape[0]):
                if e <= ex[n]:
                    np.testing.assert_allclose(al[e, n], g["logits_store"][e, n], rtol=0, atol=LOGIT_TOL)
                else:
                    assert np.isnan(al[e, n]).all()
    eng.close()


def test_tiny_per_exit_thresholds_and_temperatures(pkg, oracle):
    g = load_golden("tiny_ramp")
    cfg = pkg.ModelConfig.tiny(EE_config=TINY_CASES["tiny_ramp"])
    W = pkg.synth.make_weights(cfg, seed=int(g["seed_w"]))
    docs = {k[3:]: v for k, v in g.items() if k.startswith("in_")}
    eng = _engine(pkg, cfg, W, max_docs=8, T=int(g["text_len"]))
    E1 = g["logits_store"].shape[0]
    rng = np.random.default_rng(3)
    temps = rng.uniform(0.5, 3.0, E1)
    store = oracle.temperature_scale(g["logits_store"], temps)
    conf = oracle.softmax64(store).max(-1)
    # per-exit threshold in the widest gap between neighbouring confidences (the exit test must not be ill-posed)
    thr = np.zeros(E1)
    for e in range(E1):
        s = np.sort(conf[e])
        k = int(np.argmax(np.diff(s)))
        thr[e] = 0.5 * (s[k] + s[k + 1])
    assert np.abs(conf - thr[:, None]).min() > 1e-4
    ex, pred, cf = oracle.policy_scan(store, thr)
    out = eng.forward(docs["input_ids"], docs["attention_mask"], docs["bbox"], docs["pixel_values"], thresholds=thr,
                      temperatures=temps)
    assert np.array_equal(_np(out.exit_layer), ex)
    np.testing.assert_allclose(_np(out.logits), pred, rtol=0, atol=LOGIT_TOL)
    np.testing.assert_allclose(_np(out.confidence), cf, rtol=0, atol=1e-4)
    eng.close()


@pytest.mark.parametrize("precision", ["fp32", "split"])
def test_base_shape_matches_golden(pkg, precision):
    """Both GEMM back ends (f32 MFMA; split-f16 operands, 3 MFMA terms) against the same golden vectors, same tolerance."""
    g = load_golden("base_cls")
    cfg = pkg.ModelConfig.base(EE_config=BASE_EE)
    W = pkg.synth.make_weights(cfg, seed=int(g["seed_w"]))
    docs = pkg.synth.make_documents(cfg, int(g["n_docs"]), seed=int(g["seed_docs"]), text_len=int(g["text_len"]))
    eng = _engine(pkg, cfg, W, max_docs=4, T=512, precision=precision)
    for dense in (False, True):
        out = eng.forward(docs["input_ids"], docs["attention_mask"], docs["bbox"], docs["pixel_values"], dump_all=True,
                          dense_rows=dense, want_all=True, want_hidden_cls=True, validate=True)
        np.testing.assert_allclose(_np(out.hidden_cls), g["hidden_cls"], rtol=0, atol=1e-4)
        np.testing.assert_allclose(_np(out.all_logits), g["logits_store"], rtol=0, atol=LOGIT_TOL)
    for i in range(4):
        out = eng.forward(docs["input_ids"], docs["attention_mask"], docs["bbox"], docs["pixel_values"],
                          thresholds=float(g[f"pol_thr{i}"]))
        assert np.array_equal(_np(out.exit_layer), g[f"pol_exits{i}"])
    eng.close()


@pytest.mark.parametrize("precision", ["fp32", "split"])
@pytest.mark.parametrize("name", list(MATRIX_CASES))
def test_criterion_head_strategy_matrix_matches_golden(pkg, name, precision):
    """Entropy criterion, one-layer heads, gate strategy and the vision_avg / text_avg / text_visual_concat exits at H = 256 (the
    smallest split-precision shape) and at base shape, on both back ends, against the composed reference's vectors
    (EE/models/EE_modules.py:116-160, EE/models/LayoutLMv3.py:70-93, 465-605, 764-792); then early exit at the fixture's thresholds."""
    g = load_golden(name)
    cfg, ee, n_docs, T = matrix_config(pkg, name)
    W = pkg.synth.make_weights(cfg, seed=MATRIX_SEEDS["seed_w"])
    docs = pkg.synth.make_documents(cfg, n_docs, seed=MATRIX_SEEDS["seed_docs"], text_len=T, min_words=3)
    eng = _engine(pkg, cfg, W, max_docs=8, T=T, precision=precision)
    assert eng.precision == precision
    args = (docs["input_ids"], docs["attention_mask"], docs["bbox"], docs["pixel_values"])
    scale = max(1.0, float(np.abs(g["logits_store"]).max()))
    tol = LOGIT_TOL                                       # north star: 1e-4 ABSOLUTE, also where one-layer heads reach |logit| ~ 60 (26 ulp of f32)
    for dense in (False, True):
        out = eng.forward(*args, dump_all=True, dense_rows=dense, want_all=True, want_head=True, want_hidden_cls=True, validate=True)
        report_measured(f"matrix[{name},{precision},dense={int(dense)}]", f"max|dlogit| (max|logit| {scale:.1f})",
                        float(np.abs(_np(out.all_logits) - g["logits_store"]).max()))
        report_measured(f"matrix[{name},{precision},dense={int(dense)}]", "max|d head logit|",
                        float(np.abs(_np(out.head_logits) - g["exit_logits"]).max()))
        np.testing.assert_allclose(_np(out.hidden_cls), g["hidden_cls"], rtol=0, atol=1e-4)
        np.testing.assert_allclose(_np(out.head_logits), g["exit_logits"], rtol=0, atol=tol)
        np.testing.assert_allclose(_np(out.all_logits), g["logits_store"], rtol=0, atol=tol)
        np.testing.assert_allclose(_np(out.head_crit), g["exit_crit"], rtol=0, atol=2e-5 * scale)
    store = g["logits_store"]
    if str(cfg.exit_config.inference_strategy) == "entropy":
        # the fast path leaves at the first exit whose criterion passes its threshold with the criterion's own sign: entropy BELOW the
        # threshold (EarlyExitInference.get_sign -> operator.lt, EE/models/EE_modules.py:137-144), in float64 on the float32 logits like
        # the max-confidence test.  Thresholds in the widest gap of every exit's entropies.
        x = store.astype(np.float64)
        ent = np.log(np.exp(x).sum(-1)) - (x * np.exp(x)).sum(-1) / np.exp(x).sum(-1)           # EE/models/EE_modules.py:149-154
        E1 = ent.shape[0]
        thr = np.zeros(E1)
        margin = 1e-4 * max(1.0, float(np.abs(ent).max()))
        for e in range(E1):
            srt = np.sort(ent[e])
            k = int(np.argmax(np.diff(srt)))
            thr[e] = 0.5 * (srt[k] + srt[k + 1]) if srt[k + 1] - srt[k] > 4 * margin else -1.0      # no clear gap: nobody leaves here
        assert np.abs(ent - thr[:, None]).min() > margin
        hit = ent < thr[:, None]
        hit[-1] = True
        ex = hit.argmax(0).astype(np.int32)
        for kw in (dict(), dict(whole_layers=True), dict(probe_always=True)):
            out = eng.forward(*args, thresholds=thr, **kw)
            assert np.array_equal(_np(out.exit_layer), ex), (name, precision, kw)
            np.testing.assert_allclose(_np(out.logits), store[ex, np.arange(n_docs)], rtol=0, atol=tol)
        assert len(np.unique(ex)) >= 2
    else:
        for i in range(4):
            thr = float(g[f"pol_thr{i}"])
            if not (thr == 0.0 or thr > 1.0 or _margin_ok(store, thr, 1e-5)):
                continue
            for kw in (dict(), dict(whole_layers=True), dict(probe_always=True)):
                out = eng.forward(*args, thresholds=thr, **kw)
                assert np.array_equal(_np(out.exit_layer), g[f"pol_exits{i}"]), (name, precision, thr, kw)
                np.testing.assert_allclose(_np(out.logits), g[f"pol_pred{i}"], rtol=0, atol=tol)
    eng.close()


@pytest.mark.parametrize("precision", ["fp32", "auto"])
def test_dit_image_only_variant_matches_golden(pkg, oracle, precision):
    """BASELINE configs[4]: image-only DiT/BEiT through the same GEMM / attention / exit-compaction kernels
    ("auto" = split-f16 GEMMs at the base shape, f32 MFMA at the tiny one)."""
    from .conftest import DIT_BASE_EE, DIT_EE
    for name, mk, ee in (("dit_tiny", pkg.ModelConfig.dit_tiny, DIT_EE), ("dit_base_cls", pkg.ModelConfig.dit_base, DIT_BASE_EE)):
        g = load_golden(name)
        cfg = mk(EE_config=ee)
        W = pkg.synth.make_weights_beit(cfg, seed=int(g["seed_w"]))
        pix = pkg.synth.make_documents(cfg, int(g["n_docs"]), seed=int(g["seed_docs"]), text_len=8)["pixel_values"]
        eng = pkg.EarlyExitEngine(cfg, max_docs=8, precision=precision, xprobe=False)
        eng.load_weights(W)
        out = eng.forward(pixel_values=pix, dump_all=True, want_all=True, want_head=True, want_hidden_cls=True, validate=True)
        np.testing.assert_allclose(_np(out.hidden_cls), g["hidden_cls"], rtol=0, atol=1e-4)
        np.testing.assert_allclose(_np(out.head_logits), g["exit_logits"], rtol=0, atol=LOGIT_TOL)
        np.testing.assert_allclose(_np(out.all_logits), g["logits_store"], rtol=0, atol=LOGIT_TOL)
        if name == "dit_tiny":
            for i in range(4):
                o2 = eng.forward(pixel_values=pix, thresholds=float(g[f"pol_thr{i}"]))
                assert np.array_equal(_np(o2.exit_layer), g[f"pol_exits{i}"])
                np.testing.assert_allclose(_np(o2.logits), g[f"pol_pred{i}"], rtol=0, atol=LOGIT_TOL)
        eng.close()


def test_dit_probe_first_gives_the_same_bits(pkg, oracle):
    """Image-only DiT-base in split precision: exit layers probed first (CLS row of the pre-LN layer, decision, the rest for the documents
    that stay) against whole layers and against the dump-all rows — bit for bit; the mean-pooled last layer is never probed."""
    ee = dict(exits=[1, 2, 3], encoder_layer_strategy="ramp", inference_strategy="max_confidence")
    cfg = pkg.ModelConfig.dit_base(EE_config=ee, num_hidden_layers=4)
    W = pkg.synth.make_weights_beit(cfg, seed=21)
    B = 80
    pix = pkg.synth.make_documents(cfg, B, seed=3, text_len=8)["pixel_values"]
    eng = pkg.EarlyExitEngine(cfg, max_docs=B, precision="split", xprobe=False)
    eng.load_weights(W)
    full = eng.forward(pixel_values=pix, dump_all=True, want_all=True, want_hidden_cls=True)
    store = _np(full.all_logits).astype(np.float64)
    conf = oracle.softmax64(store).max(-1)
    thr = np.full(conf.shape[0], 2.0)
    active = np.ones(B, dtype=bool)
    for e in range(conf.shape[0] - 1):                                   # release about a third of the arrivals at every exit, in a gap
        c = np.sort(conf[e, active])
        k = int(0.66 * len(c))
        lo, hi = max(1, k - 2), min(len(c) - 1, k + 2)
        j = lo + int(np.argmax(c[lo:hi + 1] - c[lo - 1:hi]))
        thr[e] = 0.5 * (c[j - 1] + c[j])
        active &= ~(conf[e] > thr[e])
    ex_ref, _, _ = oracle.policy_scan(store, thr)
    probed = eng.forward(pixel_values=pix, thresholds=thr, probe_always=True, want_hidden_cls=True)
    sc, plan = eng.stage_counts(), eng.layer_plan()
    assert plan["docs_probe"] == [sc["docs"][0], sc["docs"][1], sc["docs"][2], 0] and plan["rows_main"] == [sc["rows"][1], sc["rows"][2], sc["rows"][3], sc["rows"][3]]
    whole = eng.forward(pixel_values=pix, thresholds=thr, whole_layers=True, want_hidden_cls=True)
    assert eng.layer_plan()["docs_probe"] == [0, 0, 0, 0]
    ex = _np(probed.exit_layer)
    assert np.array_equal(ex, ex_ref) and len(np.unique(ex)) >= 3
    assert np.array_equal(_np(whole.exit_layer), ex) and np.array_equal(_np(whole.logits), _np(probed.logits))
    assert np.array_equal(_np(probed.logits), _np(full.all_logits)[ex, np.arange(B)])          # == the dump-all rows
    a, b = _np(probed.hidden_cls), _np(whole.hidden_cls)
    assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)])
    eng.close()


def _decode_split(buf, n, scale):
    import torch
    h = buf.view(torch.float16).view(buf.shape[0], n // 16, 2, 16)      # 64-byte groups [hi 16 | lo 16]
    return (h[:, :, 0].double() + h[:, :, 1].double()).reshape(buf.shape[0], n) / scale


@pytest.mark.parametrize("M,N,K,epi,out_split,gather", [
    (1, 256, 32, 0, 0, False),          # single row, single k-stage
    (130, 256, 96, 0, 0, False),        # ragged last tile, three k-stages (ring start-up)
    (300, 512, 768, 2, 0, True),        # residual + gathered A / residual rows (the layer after an exit)
    (257, 1024, 256, 1, 1, False),      # GELU, split-row output (FFN-up -> FFN-down hand-over)
    (512, 768, 3072, 3, 0, False),      # tanh, long K
])
def test_split_gemm_kernel_against_float64(pkg, M, N, K, epi, out_split, gather):
    """The split-precision GEMM kernel alone: |error| vs an f64 reference no worse than 2x a plain f32 GEMM's."""
    import ctypes as C
    import torch
    lib = pkg.capi.load()
    dev = torch.device("cuda:0")
    gen = torch.Generator(device="cpu").manual_seed(M * 131 + N + K)
    rows_A = M + 40 if gather else M
    A = torch.randn(rows_A, K, generator=gen).to(dev)
    W = (torch.randn(N, K, generator=gen) * 0.02).to(dev)
    b = torch.randn(N, generator=gen).to(dev)
    R = torch.randn(rows_A, N, generator=gen).to(dev) if epi == 2 else None
    rs = torch.sort(torch.randperm(rows_A, generator=gen)[:M]).values.to(torch.int32).to(dev) if gather else None
    out = torch.full((M, N), float("nan"), device=dev)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    pkg.capi.check(lib.ee_debug_gemm_split(p(A), p(W), p(b), p(R), p(out), M, N, K, epi, out_split, 16.0, 256.0, 16.0, p(rs), rows_A, 1,
                                           None, C.c_void_p(torch.cuda.current_stream().cuda_stream)), None, "ee_debug_gemm_split")
    torch.cuda.synchronize()
    Ag = A[rs.long()] if gather else A
    ref = Ag.double() @ W.double().t() + b.double()
    f32 = Ag @ W.t() + b
    if epi == 1: ref, f32 = torch.nn.functional.gelu(ref), torch.nn.functional.gelu(f32)
    if epi == 2: ref, f32 = ref + R[rs.long()].double() if gather else ref + R.double(), f32 + (R[rs.long()] if gather else R)
    if epi == 3: ref, f32 = torch.tanh(ref), torch.tanh(f32)
    got = _decode_split(out, N, 16.0) if out_split else out.double()
    err = float((got - ref).abs().max())
    err32 = float((f32.double() - ref).abs().max())
    assert err <= max(2.0 * err32, 1e-6), (err, err32)


@pytest.mark.parametrize("strategy", ["ramp", "gate"])
def test_small_split_precision_every_exit_kind_vs_oracle(pkg, oracle, strategy):
    """Split-precision GEMM / attention kernels at the smallest shape they accept (hidden 256), every exit kind
    (embedding-level means + encoder layers, ramp and gate), dump-all and early-exit mode, against the live numpy oracle."""
    ee = dict(exits=["vision_avg", "text_avg", "text_visual_concat", 1, 2, 3], encoder_layer_strategy=strategy)
    cfg = pkg.ModelConfig.tiny(EE_config=ee, hidden_size=256, num_attention_heads=4, intermediate_size=512, num_hidden_layers=3,
                               coordinate_size=48, shape_size=32)
    W = pkg.synth.make_weights(cfg, seed=21)
    docs = pkg.synth.make_documents(cfg, 7, seed=5, text_len=40, min_words=2)
    ref = oracle.forward_all(cfg, W, docs, ee["exits"], strategy=strategy, return_hidden_cls=True)
    eng = pkg.EarlyExitEngine(cfg, max_docs=8, max_text_len=40, precision="split", xprobe=False)
    assert eng.precision == "split"
    eng.load_weights(W)
    out = eng.forward(docs["input_ids"], docs["attention_mask"], docs["bbox"], docs["pixel_values"], dump_all=True, want_all=True,
                      want_hidden_cls=True, validate=True)
    np.testing.assert_allclose(_np(out.hidden_cls), ref["hidden_cls"], rtol=0, atol=5e-5)
    np.testing.assert_allclose(_np(out.all_logits), ref["logits_store"], rtol=0, atol=LOGIT_TOL)
    conf = oracle.softmax64(ref["logits_store"]).max(-1)
    s = np.sort(conf.ravel())
    k = int(np.argmax(np.diff(s)[len(s) // 4: 3 * len(s) // 4])) + len(s) // 4     # widest gap in the middle half
    thr = 0.5 * (s[k] + s[k + 1])
    assert np.abs(conf - thr).min() > 1e-5
    ex, pred, cf = oracle.policy_scan(ref["logits_store"], thr)
    for dense in (False, True):
        o2 = eng.forward(docs["input_ids"], docs["attention_mask"], docs["bbox"], docs["pixel_values"], thresholds=thr, dense_rows=dense)
        assert np.array_equal(_np(o2.exit_layer), ex)
        np.testing.assert_allclose(_np(o2.logits), pred, rtol=0, atol=LOGIT_TOL)
    eng.close()


@pytest.mark.parametrize("bins", [(32, 128), (128, 64)])
def test_wide_bucket_tables_run_the_delta_table_attention(pkg, oracle, bins):
    """Bucket tables beyond 64 bins do not fit the pair index (6-bit fields): the split precision then runs csrc/attention_pair.hip (clamped
    Delta tables gathered per layer and head) -- a PRODUCT kernel that no other test reaches.  Same checks as the test above:
    relative_position_bucket with num_buckets = 128 (HF:392-413), dump-all and early exit against the live oracle, both row layouts."""
    ee = dict(exits=["text_visual_concat", 1, 2, 3], encoder_layer_strategy="ramp")
    cfg = pkg.ModelConfig.tiny(EE_config=ee, hidden_size=256, num_attention_heads=4, intermediate_size=512, num_hidden_layers=3,
                               coordinate_size=48, shape_size=32, rel_pos_bins=bins[0], rel_2d_pos_bins=bins[1])
    W = pkg.synth.make_weights(cfg, seed=22)
    docs = pkg.synth.make_documents(cfg, 6, seed=6, text_len=40, min_words=2)
    ref = oracle.forward_all(cfg, W, docs, ee["exits"], strategy="ramp", return_hidden_cls=True)
    eng = pkg.EarlyExitEngine(cfg, max_docs=8, max_text_len=40, precision="split", xprobe=False)
    assert eng.precision == "split"
    eng.load_weights(W)
    args = (docs["input_ids"], docs["attention_mask"], docs["bbox"], docs["pixel_values"])
    out = eng.forward(*args, dump_all=True, want_all=True, want_hidden_cls=True, validate=True)
    np.testing.assert_allclose(_np(out.hidden_cls), ref["hidden_cls"], rtol=0, atol=5e-5)
    np.testing.assert_allclose(_np(out.all_logits), ref["logits_store"], rtol=0, atol=LOGIT_TOL)
    conf = oracle.softmax64(ref["logits_store"]).max(-1)
    srt = np.sort(conf.ravel())
    k = int(np.argmax(np.diff(srt)[len(srt) // 4: 3 * len(srt) // 4])) + len(srt) // 4
    thr = 0.5 * (srt[k] + srt[k + 1])
    assert np.abs(conf - thr).min() > 1e-5
    ex, pred, _ = oracle.policy_scan(ref["logits_store"], thr)
    for dense in (False, True):
        for kw in (dict(), dict(whole_layers=True), dict(probe_always=True)):
            o2 = eng.forward(*args, thresholds=thr, dense_rows=dense, validate=True, **kw)
            assert np.array_equal(_np(o2.exit_layer), ex)
            np.testing.assert_allclose(_np(o2.logits), pred, rtol=0, atol=LOGIT_TOL)
    eng.close()


def test_wide_bucket_tables_mask_holes_in_full_key_tiles(pkg, oracle):
    """csrc/attention_pair.hip and holes in the attention mask (the two tests above and test_gpu_round6.py's holes test never met): a hole stays a
    row, masked as a key, and the pair kernel's fast key tiles never read a key's flags -- so whether a document takes them must follow from
    the document (a per-document word the row-metadata pass raises), not from MMEE_FLAG_DENSE_ROWS.  Holes inside FULL 32-key tiles, both row
    layouts, against the live oracle."""
    ee = dict(exits=["text_visual_concat", 1, 2, 3], encoder_layer_strategy="ramp")
    cfg = pkg.ModelConfig.tiny(EE_config=ee, hidden_size=256, num_attention_heads=4, intermediate_size=512, num_hidden_layers=3,
                               coordinate_size=48, shape_size=32, rel_pos_bins=128, rel_2d_pos_bins=64)
    W = pkg.synth.make_weights(cfg, seed=22)
    docs = pkg.synth.make_documents(cfg, 6, seed=22, text_len=64, min_words=20)
    rng = np.random.default_rng(5)
    am = docs["attention_mask"]
    in_full_tile = 0
    for b in range(6):                                   # holes in the valid range (never position 0), one document masked almost entirely
        n = int(am[b].sum())
        holes = rng.choice(np.arange(1, n - 1), size=(n - 3) if b == 5 else max(1, n // 4), replace=False)
        am[b, holes] = 0
        rows = int(np.nonzero(am[b])[0].max()) + 1 + 17    # the prefix up to the last kept token + (64 / 16)^2 + 1 visual rows
        in_full_tile += int(((holes // 32 + 1) * 32 <= rows).sum())
    assert in_full_tile >= 6
    ref = oracle.forward_all(cfg, W, docs, ee["exits"], strategy="ramp")
    eng = pkg.EarlyExitEngine(cfg, max_docs=6, max_text_len=64, precision="split", xprobe=False)
    assert eng.precision == "split"
    eng.load_weights(W)
    args = (docs["input_ids"], docs["attention_mask"], docs["bbox"], docs["pixel_values"])
    errs = {}
    for dense in (False, True):
        out = eng.forward(*args, dump_all=True, want_all=True, validate=True, dense_rows=dense)
        errs[dense] = float(np.abs(_np(out.all_logits) - ref["logits_store"]).max())
        report_measured(f"wide_buckets_holes[dense={int(dense)}]", "max|dlogit| vs oracle", errs[dense])
    eng.close()
    assert errs[False] <= LOGIT_TOL and errs[True] <= LOGIT_TOL, errs


@pytest.mark.parametrize("precision", ["split", "fp32"])
def test_bench_size_early_exit_properties(pkg, oracle, precision):
    """BASELINE configs[1] shape (base, exits 2/4/6/8/10 + final, T = 512, ragged documents) at a size no CPU oracle
    finishes in seconds — checked through properties that do not depend on the size:
      * a document's early-exit result is BIT-identical to its dump-all result at the exit the policy picks (rows are
        independent in every kernel, so dropping the other documents must not change a single bit);
      * permuting the batch permutes the outputs bit for bit (work queues, compaction and tiling are order-free);
      * the stage populations are the survivors of the exits, and every document leaves exactly once;
      * split precision runs exit layers "probe first" (CLS rows, decision, then the layer's bulk for the documents that stay):
        the whole-layer run (`whole_layers=True`, what the reference does) gives the same bits, and the layer plan says which
        rows each layer really processed."""
    import torch
    ee = dict(exits=[2, 4, 6, 8, 10], encoder_layer_strategy="ramp")
    cfg = pkg.ModelConfig.base(EE_config=ee)
    W = pkg.synth.make_weights(cfg, seed=1234, head_gain=6.0)          # bench.py's gain: confidences spread over (0.2, 1)
    B = 160
    docs = pkg.synth.make_documents(cfg, B, seed=99, text_len=512)
    eng = pkg.EarlyExitEngine(cfg, max_docs=B, max_text_len=512, precision=precision, xprobe=False)
    eng.load_weights(W)
    args = (docs["input_ids"], docs["attention_mask"], docs["bbox"], docs["pixel_values"])
    full = eng.forward(*args, dump_all=True, want_all=True)
    store = _np(full.all_logits).astype(np.float64)                     # (E+1, B, K)
    conf = oracle.softmax64(store).max(-1)
    thr = np.full(conf.shape[0], 2.0)
    active = np.ones(B, dtype=bool)
    for e in range(conf.shape[0] - 1):                                   # release ~25 % of the arrivals at every exit, in a gap
        c = np.sort(conf[e, active])
        k = int(0.75 * len(c))
        lo, hi = max(1, k - 3), min(len(c) - 1, k + 3)
        j = lo + int(np.argmax(c[lo:hi + 1] - c[lo - 1:hi]))
        thr[e] = 0.5 * (c[j - 1] + c[j])
        active &= ~(conf[e] > thr[e])
    assert np.abs(conf[:-1] - thr[:-1, None]).min() > 1e-6
    ex_ref, pred_ref, _ = oracle.policy_scan(store, thr)
    out = eng.forward(*args, thresholds=thr, probe_always=True)
    ex = _np(out.exit_layer)
    assert np.array_equal(ex, ex_ref)
    assert len(np.unique(ex)) >= 4                                       # the mix really exercises several stages
    got = _np(out.logits)
    want = _np(full.all_logits)[ex, np.arange(B)]
    assert np.array_equal(got, want), float(np.abs(got - want).max())    # bit-identical to the dump-all rows
    sc = eng.stage_counts()
    counts = sc["docs"]
    surv = [int((ex >= e).sum()) for e in range(len(counts))]
    assert counts == surv and sum(int((ex == e).sum()) for e in range(conf.shape[0])) == B
    # probe-first exit layers: which rows each layer processed, and the whole-layer run as the A/B
    plan = eng.layer_plan()
    stage_before = [sum(1 for x in ee["exits"] if x <= l) for l in range(cfg.num_hidden_layers)]      # stage entering layer l
    assert plan["rows_qkv"] == [sc["rows"][st] for st in stage_before]
    if precision == "split":
        for l in range(cfg.num_hidden_layers):
            ends_in_decision = (l + 1) in ee["exits"] or l == cfg.num_hidden_layers - 1
            assert plan["docs_probe"][l] == (sc["docs"][stage_before[l]] if ends_in_decision else 0)
            want_rows = 0 if l == cfg.num_hidden_layers - 1 else sc["rows"][stage_before[l] + (1 if (l + 1) in ee["exits"] else 0)]
            assert plan["rows_main"][l] == want_rows, (l, plan)
        assert plan["probe_flops"] > 0
    else:
        assert plan["docs_probe"] == [0] * cfg.num_hidden_layers and plan["rows_main"] == plan["rows_qkv"]
    whole = eng.forward(*args, thresholds=thr, whole_layers=True, want_hidden_cls=True)
    assert eng.layer_plan()["docs_probe"] == [0] * cfg.num_hidden_layers
    assert np.array_equal(_np(whole.exit_layer), ex) and np.array_equal(_np(whole.logits), got)
    assert np.array_equal(_np(whole.confidence), _np(out.confidence))
    hid = eng.forward(*args, thresholds=thr, want_hidden_cls=True, probe_always=True)
    a, b = _np(hid.hidden_cls), _np(whole.hidden_cls)
    assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)])   # CLS of every layer, every active document
    # permutation invariance
    perm = np.random.default_rng(7).permutation(B)
    pargs = tuple(a[perm] for a in args)
    outp = eng.forward(*pargs, thresholds=thr)
    assert np.array_equal(_np(outp.exit_layer), ex[perm])
    assert np.array_equal(_np(outp.logits), got[perm])
    assert np.array_equal(_np(outp.confidence), _np(out.confidence)[perm])
    eng.close()


def test_xspace_probe_matches_whole_layers_and_goldens(pkg, oracle):
    """MMEE_FLAG_XPROBE (csrc/xprobe.hip): probe-first layers take the CLS context in X space and project Q | K | V only for the documents
    that stay (HF:235-288 re-associated: (W_k^T q) . x_j and W_v sum_j p_j x_j).  Same exit indices, logits within the 1e-4 bar of the
    whole-layer run, of the composed reference's vectors (base shape) and CLS rows; the layer plan shows the projection shrinking."""
    # (1) base-shape golden vectors
    g = load_golden("base_cls")
    cfg = pkg.ModelConfig.base(EE_config=BASE_EE)
    W = pkg.synth.make_weights(cfg, seed=int(g["seed_w"]))
    docs = pkg.synth.make_documents(cfg, int(g["n_docs"]), seed=int(g["seed_docs"]), text_len=int(g["text_len"]))
    eng0 = eng = _engine(pkg, cfg, W, max_docs=4, T=512, precision="split")
    args = (docs["input_ids"], docs["attention_mask"], docs["bbox"], docs["pixel_values"])
    for dense in (False, True):
        for i in range(4):
            out = eng.forward(*args, thresholds=float(g[f"pol_thr{i}"]), xprobe=True, probe_always=True, dense_rows=dense, want_hidden_cls=True,
                              validate=True)
            ex = _np(out.exit_layer)
            assert np.array_equal(ex, g[f"pol_exits{i}"]), (i, dense)
            np.testing.assert_allclose(_np(out.logits), g[f"pol_pred{i}"], rtol=0, atol=LOGIT_TOL)
            hc = _np(out.hidden_cls)
            ok = ~np.isnan(hc)
            np.testing.assert_allclose(hc[ok], g["hidden_cls"][ok], rtol=0, atol=1e-4)
            # (documents that left at the embedding exit are never probed: docs_probe may be all zero for a low threshold)
            assert sum(eng.layer_plan()["docs_probe"]) > 0 or (ex < 1).all()
    # (1b) empty stages: every document leaves at the embedding exit, so each probe of the encoder runs on zero documents (the ticket
    # counter of the probe kernel must not depend on what the workspace held before: tools/fuzz_schedules.py, round 3)
    for _ in range(2):
        out = eng0.forward(*args, thresholds=0.0, xprobe=True, probe_always=True, validate=True)
        assert (_np(out.exit_layer) == 0).all() and eng0.layer_plan()["rows_qkv"] == [0] * cfg.num_hidden_layers
    eng0.close()
    # (2) bench shape, 160 ragged documents: exits equal to the whole-layer run with thresholds in gaps, logits within tolerance, and the
    # Q | K | V projection of an exit layer runs on the rows that STAY (none in the last layer)
    ee = dict(exits=[2, 4, 6, 8, 10], encoder_layer_strategy="ramp")
    cfg = pkg.ModelConfig.base(EE_config=ee)
    W = pkg.synth.make_weights(cfg, seed=1234, head_gain=6.0)
    B = 160
    docs = pkg.synth.make_documents(cfg, B, seed=99, text_len=512)
    eng = pkg.EarlyExitEngine(cfg, max_docs=B, max_text_len=512, precision="split", xprobe=False)
    eng.load_weights(W)
    args = (docs["input_ids"], docs["attention_mask"], docs["bbox"], docs["pixel_values"])
    full = eng.forward(*args, dump_all=True, want_all=True)
    store = _np(full.all_logits).astype(np.float64)
    conf = oracle.softmax64(store).max(-1)
    thr = np.full(conf.shape[0], 2.0)
    active = np.ones(B, dtype=bool)
    for e in range(conf.shape[0] - 1):
        c = np.sort(conf[e, active])
        k = int(0.75 * len(c))
        lo, hi = max(1, k - 3), min(len(c) - 1, k + 3)
        j = lo + int(np.argmax(c[lo:hi + 1] - c[lo - 1:hi]))
        thr[e] = 0.5 * (c[j - 1] + c[j])
        active &= ~(conf[e] > thr[e])
    assert np.abs(conf[:-1] - thr[:-1, None]).min() > 1e-5               # gaps wider than the re-association noise
    whole = eng.forward(*args, thresholds=thr, whole_layers=True, want_hidden_cls=True)
    xp = eng.forward(*args, thresholds=thr, xprobe=True, probe_always=True, want_hidden_cls=True, validate=True)
    sc, plan = eng.stage_counts(), eng.layer_plan()
    assert np.array_equal(_np(xp.exit_layer), _np(whole.exit_layer))
    np.testing.assert_allclose(_np(xp.logits), _np(whole.logits), rtol=0, atol=LOGIT_TOL)
    np.testing.assert_allclose(_np(xp.confidence), _np(whole.confidence), rtol=0, atol=1e-4)
    a, b = _np(xp.hidden_cls), _np(whole.hidden_cls)
    assert np.array_equal(np.isnan(a), np.isnan(b))
    assert float(np.abs(a[~np.isnan(a)] - b[~np.isnan(b)]).max()) < 1e-4
    stage_before = [sum(1 for x in ee["exits"] if x <= l) for l in range(cfg.num_hidden_layers)]
    for l in range(cfg.num_hidden_layers):
        last = l == cfg.num_hidden_layers - 1
        exit_here = (l + 1) in ee["exits"]
        want_qkv = 0 if last else sc["rows"][stage_before[l] + (1 if exit_here else 0)]       # projected AFTER the decision: the rows that stay
        assert plan["rows_qkv"][l] == want_qkv, (l, plan["rows_qkv"], sc)
        assert plan["rows_main"][l] == want_qkv
        assert plan["docs_probe"][l] == (sc["docs"][stage_before[l]] if (exit_here or last) else 0)
    # the default schedule with xprobe gives the same exits too
    d2 = eng.forward(*args, thresholds=thr, xprobe=True)
    assert np.array_equal(_np(d2.exit_layer), _np(whole.exit_layer))
    eng.close()


def test_exit_layer_schedule_is_pinned_never_inferred(pkg, oracle):
    """Round 5.  Rounds 2-4 let ee_forward decide per exit layer whether to probe first from the stage populations of the
    handle's most recent FINISHED forward -- a timing-dependent choice.  Now the schedule is part of the handle's configuration: every layer
    that ends in a decision by default, whatever ran before (many leavers, hardly any, a dump); the cost model is an explicit query
    (pin_schedule() -> ee_suggest_probe_mask) whose answer the caller pins; MMEE_FLAG_WHOLE_LAYERS / PROBE_ALWAYS override a pinned mask; and
    the results are the same bits in every schedule."""
    ee = dict(exits=[2], encoder_layer_strategy="ramp")
    cfg = pkg.ModelConfig.base(EE_config=ee, num_hidden_layers=4)
    W = pkg.synth.make_weights(cfg, seed=11, head_gain=6.0)
    B = 96
    docs = pkg.synth.make_documents(cfg, B, seed=5, text_len=128)
    eng = pkg.EarlyExitEngine(cfg, max_docs=B, max_text_len=128, precision="split", xprobe=False)
    eng.load_weights(W)
    args = (docs["input_ids"], docs["attention_mask"], docs["bbox"], docs["pixel_values"])
    full = eng.forward(*args, dump_all=True, want_all=True)
    conf = oracle.softmax64(_np(full.all_logits).astype(np.float64)).max(-1)[0]
    c = np.sort(conf)

    def gap(k):                                   # a threshold that releases the B - k most confident documents at the exit
        lo, hi = max(1, k - 2), min(B - 1, k + 2)
        j = lo + int(np.argmax(c[lo:hi + 1] - c[lo - 1:hi]))
        return 0.5 * (c[j - 1] + c[j]), B - j

    thr_many, n_many = gap(B // 2)                # about half of the documents leave at layer 2
    thr_few, n_few = gap(B - 2)                   # two or so leave
    first = eng.forward(*args, thresholds=[thr_many, 2.0])
    assert eng.layer_plan()["docs_probe"] == [0, B, 0, B - n_many]
    many = eng.forward(*args, thresholds=[thr_many, 2.0])
    assert eng.layer_plan()["docs_probe"] == [0, B, 0, B - n_many] and eng.stage_counts()["docs"] == [B, B - n_many]
    assert eng.pin_schedule() == [1]              # asked: half leave -> the probe pays; pinned
    few = eng.forward(*args, thresholds=[thr_few, 2.0])
    assert eng.layer_plan()["docs_probe"] == [0, B, 0, B - n_few]       # pinned: what earlier forwards did changes nothing
    assert eng.pin_schedule() == []               # asked again: almost nobody leaves -> layer 2 should run whole; pinned
    few2 = eng.forward(*args, thresholds=[thr_few, 2.0])
    assert eng.layer_plan()["docs_probe"] == [0, 0, 0, B - n_few]       # ... the last layer is the probe alone either way
    many2 = eng.forward(*args, thresholds=[thr_many, 2.0])
    assert eng.layer_plan()["docs_probe"] == [0, 0, 0, B - n_many]      # still pinned, although half of the documents leave again
    always = eng.forward(*args, thresholds=[thr_few, 2.0], probe_always=True)
    assert eng.layer_plan()["docs_probe"] == [0, B, 0, B - n_few]
    assert eng.pin_schedule(False) is None
    dflt = eng.forward(*args, thresholds=[thr_few, 2.0])
    assert eng.layer_plan()["docs_probe"] == [0, B, 0, B - n_few]       # the default again: every decision layer
    whole = eng.forward(*args, thresholds=[thr_few, 2.0], whole_layers=True)
    assert eng.layer_plan()["docs_probe"] == [0, 0, 0, 0]
    for a, b in ((first, many), (many, many2), (few, few2), (few, whole), (few, always), (few, dflt)):
        assert np.array_equal(_np(a.exit_layer), _np(b.exit_layer)) and np.array_equal(_np(a.logits), _np(b.logits))
        assert np.array_equal(_np(a.confidence), _np(b.confidence))
    assert int((_np(many.exit_layer) == 0).sum()) == n_many and int((_np(few.exit_layer) == 0).sum()) == n_few
    eng.close()


def test_split_precision_edge_batches(pkg, oracle):
    """Split-precision path at the base width on degenerate batches: one document, everybody leaving at the first exit (every
    later stage is empty: M = 0 launches), nobody leaving, short texts; a batch larger than the handle is refused loudly."""
    ee = dict(exits=[1, 2], encoder_layer_strategy="ramp")
    cfg = pkg.ModelConfig.base(EE_config=ee, num_hidden_layers=3)
    W = pkg.synth.make_weights(cfg, seed=3, head_gain=6.0)
    docs = pkg.synth.make_documents(cfg, 5, seed=8, text_len=24, min_words=1)
    args = (docs["input_ids"], docs["attention_mask"], docs["bbox"], docs["pixel_values"])
    eng = pkg.EarlyExitEngine(cfg, max_docs=5, max_text_len=24, precision="split", xprobe=False)
    eng.load_weights(W)
    with pytest.raises(pkg.capi.MMEEError):
        eng.forward(*(np.concatenate([a, a]) for a in args), dump_all=True)   # 10 documents, handle sized for 5
    full = eng.forward(*args, dump_all=True, want_all=True)
    store = _np(full.all_logits)
    assert np.isfinite(store).all()
    one = eng.forward(*(a[:1] for a in args), dump_all=True, want_all=True)
    assert np.array_equal(_np(one.all_logits)[:, 0], store[:, 0])        # a document alone == the same document in a batch
    everybody = eng.forward(*args, thresholds=0.0)
    assert (_np(everybody.exit_layer) == 0).all() and np.array_equal(_np(everybody.logits), store[0])
    nobody = eng.forward(*args, thresholds=1.5)
    assert (_np(nobody.exit_layer) == 2).all() and np.array_equal(_np(nobody.logits), store[2])
    ref = oracle.forward_all(cfg, W, docs, ee["exits"])
    np.testing.assert_allclose(store, ref["logits_store"], rtol=0, atol=LOGIT_TOL)
    eng.close()


def test_baseline_config1_64_documents_threshold_sweep(pkg, oracle):
    """BASELINE configs[0], the reference's own CPU-runnable case: LayoutLMv3-base, the repo-default exits
    ["text_visual_concat", 6] (EE/configs.py:52) + final, ramp, 64 documents, a sweep of global thresholds that includes the
    repo default 0.9 (EE/configs.py:51).  The CPU side is the torch-CPU restatement of the reference path (B = 1 per forward,
    full depth, policy simulated afterwards, as the reference evaluates); the GPU side really exits."""
    import importlib
    import torch
    otorch = importlib.import_module("oracle.ee_oracle_torch")
    ee = dict(exits=["text_visual_concat", 6], encoder_layer_strategy="ramp", global_threshold=0.9)
    cfg = pkg.ModelConfig.base(EE_config=ee)
    W = pkg.synth.make_weights(cfg, seed=51, head_gain=6.0)
    N = 64
    docs = pkg.synth.make_documents(cfg, N, seed=52, text_len=512)
    torch.set_num_threads(min(16, torch.get_num_threads()))
    tor = otorch.TorchOracle(cfg, W)
    store = np.concatenate([tor.forward_all({k: v[i:i + 1] for k, v in docs.items()}, ee["exits"])["logits_store"] for i in range(N)], axis=1)
    conf = oracle.softmax64(store).max(-1)
    eng = pkg.EarlyExitEngine(cfg, max_docs=N, max_text_len=512, xprobe=False)         # precision "auto" -> split at this shape
    assert eng.precision == "split"
    eng.load_weights(W)
    args = (docs["input_ids"], docs["attention_mask"], docs["bbox"], docs["pixel_values"])
    full = eng.forward(*args, dump_all=True, want_all=True)
    np.testing.assert_allclose(_np(full.all_logits), store, rtol=0, atol=LOGIT_TOL)
    checked = 0
    for thr in (0.0, 0.3, 0.5, 0.7, 0.9, 0.99, 1.0 + 1e-6):
        if 0.0 < thr < 1.0 and np.abs(conf[:-1] - thr).min() < 2e-5:    # ill-posed: a confidence sits on the threshold
            continue
        ex, pred, _ = oracle.policy_scan(store, thr)
        for kw in (dict(xprobe=False), dict(xprobe=True, probe_always=True)):         # the K | V probe and the X-space probe (MMEE_FLAG_XPROBE)
            out = eng.forward(*args, thresholds=thr, **kw)
            assert np.array_equal(_np(out.exit_layer), ex), (thr, kw)
            np.testing.assert_allclose(_np(out.logits), pred, rtol=0, atol=LOGIT_TOL)
        checked += 1
    assert checked >= 5
    eng.close()


def test_xspace_probe_config2_exit_set_32_documents_vs_cpu_restatement(pkg, oracle):
    """The path the bench line runs (MMEE_FLAG_XPROBE, BASELINE configs[1]: LayoutLMv3-base, exits 2/4/6/8/10 + final, ramp, T = 512)
    against the torch-CPU restatement of the reference path on 32 ragged documents: per-exit thresholds in gaps that release about a
    quarter of the documents reaching each exit, so all six stages are populated; exit indices equal, logits within 1e-4 abs, for the
    X-space probe (flagged at every exit layer and under the default schedule -- since round 5 the same thing), the K | V probe and whole layers."""
    import importlib
    import torch
    otorch = importlib.import_module("oracle.ee_oracle_torch")
    ee = dict(exits=[2, 4, 6, 8, 10], encoder_layer_strategy="ramp")
    cfg = pkg.ModelConfig.base(EE_config=ee)
    W = pkg.synth.make_weights(cfg, seed=1234, head_gain=6.0)
    N = 32
    docs = pkg.synth.make_documents(cfg, N, seed=77, text_len=512)
    torch.set_num_threads(min(16, torch.get_num_threads()))
    tor = otorch.TorchOracle(cfg, W)
    store = np.concatenate([tor.forward_all({k: v[i:i + 1] for k, v in docs.items()}, ee["exits"])["logits_store"] for i in range(N)], axis=1)
    conf = oracle.softmax64(store).max(-1)
    E1 = conf.shape[0]
    thr = np.full(E1, 2.0)
    active = np.ones(N, dtype=bool)
    for e in range(E1 - 1):
        c = np.sort(conf[e, active])
        if len(c) < 4:
            continue
        k = int(0.75 * len(c))
        lo, hi = max(1, k - 2), min(len(c) - 1, k + 2)
        j = lo + int(np.argmax(c[lo:hi + 1] - c[lo - 1:hi]))
        thr[e] = 0.5 * (c[j - 1] + c[j])
        active &= ~(conf[e] > thr[e])
    assert np.abs(conf[:-1] - thr[:-1, None]).min() > 2e-5
    ex, pred, _ = oracle.policy_scan(store, thr)
    assert len(np.unique(ex)) >= 5                                       # the stages are really populated
    eng = pkg.EarlyExitEngine(cfg, max_docs=N, max_text_len=512, xprobe=False)
    assert eng.precision == "split"
    eng.load_weights(W)
    args = (docs["input_ids"], docs["attention_mask"], docs["bbox"], docs["pixel_values"])
    full = eng.forward(*args, dump_all=True, want_all=True, validate=True)
    report_measured("config2_32docs[dump-all]", "max|dlogit| vs torch-CPU", float(np.abs(_np(full.all_logits) - store).max()))
    np.testing.assert_allclose(_np(full.all_logits), store, rtol=0, atol=LOGIT_TOL)
    for tag, kw in (("xprobe,probe_always", dict(xprobe=True, probe_always=True)), ("xprobe", dict(xprobe=True)),
                    ("kv probe_always", dict(probe_always=True)), ("whole_layers", dict(whole_layers=True))):
        for dense in (False, True):
            out = eng.forward(*args, thresholds=thr, dense_rows=dense, validate=True, **kw)
            assert np.array_equal(_np(out.exit_layer), ex), (tag, dense)
            err = float(np.abs(_np(out.logits) - pred).max())
            report_measured(f"config2_32docs[{tag},dense={int(dense)}]", "max|dlogit| vs torch-CPU", err)
            assert err < LOGIT_TOL, (tag, dense, err)
    eng.close()


def test_custom_position_ids_and_defaulted_mask_and_bbox_vs_oracle(pkg, oracle):
    """Inputs the reference signature accepts and the evaluation loop never passes (EE/models/LayoutLMv3.py:425-436, 490-517):
    caller-supplied position_ids (they reach the position-embedding lookup only: the 1-D relative bias uses arange(T), :559-563),
    attention_mask=None (-> ones: pad tokens become keys) and bbox=None (-> zeros), through the C-ABI against oracle.forward_all, in both
    precisions at the smallest split-precision shape, dump-all and early exit."""
    ee = dict(exits=["text_avg", "text_visual_concat", 1, 2], encoder_layer_strategy="ramp")
    from .conftest import H256_KW
    cfg = pkg.ModelConfig.tiny(EE_config=ee, **H256_KW)
    W = pkg.synth.make_weights(cfg, seed=41, head_gain=6.0)
    B, T = 6, 48
    docs = pkg.synth.make_documents(cfg, B, seed=42, text_len=T, min_words=3)
    rng = np.random.default_rng(43)
    pos = rng.integers(2, cfg.max_position_embeddings, size=(B, T)).astype(np.int64)      # arbitrary, not the pad-aware cumsum of HF:138-146
    cases = {
        "position_ids": dict(docs, position_ids=pos),
        "mask=None": {k: v for k, v in docs.items() if k != "attention_mask"},
        "bbox=None": dict({k: v for k, v in docs.items() if k != "bbox"}, bbox=np.zeros((B, T, 4), dtype=np.int64)),
        "all three": dict({k: v for k, v in docs.items() if k not in ("attention_mask", "bbox")}, position_ids=pos,
                          bbox=np.zeros((B, T, 4), dtype=np.int64)),
    }
    for precision in ("fp32", "split"):
        eng = pkg.EarlyExitEngine(cfg, max_docs=B, max_text_len=T, precision=precision, xprobe=False)
        eng.load_weights(W)
        for tag, batch in cases.items():
            ref = oracle.forward_all(cfg, W, batch, ee["exits"])
            kw = dict(input_ids=batch["input_ids"], attention_mask=batch.get("attention_mask"), pixel_values=batch["pixel_values"],
                      bbox=None if "bbox" in tag or tag == "all three" else batch["bbox"], position_ids=batch.get("position_ids"))
            out = eng.forward(**kw, dump_all=True, want_all=True, validate=True)
            err = float(np.abs(_np(out.all_logits) - ref["logits_store"]).max())
            report_measured(f"nondefault_inputs[{tag},{precision}]", "max|dlogit|", err)
            assert err < LOGIT_TOL, (tag, precision, err)
            conf = oracle.softmax64(ref["logits_store"]).max(-1)
            srt = np.sort(conf, axis=1)
            thr = 0.5 * (srt[:, B // 2 - 1] + srt[:, B // 2])
            if np.abs(conf - thr[:, None]).min() < 1e-5:
                continue
            ex, pred, _ = oracle.policy_scan(ref["logits_store"], thr)
            o2 = eng.forward(**kw, thresholds=thr, validate=True)
            assert np.array_equal(_np(o2.exit_layer), ex), (tag, precision)
            np.testing.assert_allclose(_np(o2.logits), pred, rtol=0, atol=LOGIT_TOL)
        # the defaulted inputs really change the result (the test would be vacuous otherwise)
        a = oracle.forward_all(cfg, W, cases["position_ids"], ee["exits"])["logits_store"]
        b = oracle.forward_all(cfg, W, docs, ee["exits"])["logits_store"]
        assert np.abs(a - b).max() > 1e-3
        eng.close()


def test_engine_default_is_the_xspace_probe(pkg, oracle):
    """EarlyExitEngine() with no xprobe argument runs the X-space CLS probe at probe-first layers where the library has it (split precision,
    LayoutLMv3 shapes: the schedule bench.py measures) and the K | V probe elsewhere; xprobe=False pins the bit-identical K | V probe."""
    g = load_golden("base_cls")
    cfg = pkg.ModelConfig.base(EE_config=BASE_EE)
    W = pkg.synth.make_weights(cfg, seed=int(g["seed_w"]))
    docs = pkg.synth.make_documents(cfg, int(g["n_docs"]), seed=int(g["seed_docs"]), text_len=int(g["text_len"]))
    args = (docs["input_ids"], docs["attention_mask"], docs["bbox"], docs["pixel_values"])
    eng = pkg.EarlyExitEngine(cfg, max_docs=4, max_text_len=512)
    assert eng.precision == "split" and eng.xprobe_default is True
    eng.load_weights(W)
    i = max(range(4), key=lambda k: len(np.unique(g[f"pol_exits{k}"])))          # the threshold with the most varied exits
    out = eng.forward(*args, thresholds=float(g[f"pol_thr{i}"]), probe_always=True, validate=True)
    assert np.array_equal(_np(out.exit_layer), g[f"pol_exits{i}"])
    np.testing.assert_allclose(_np(out.logits), g[f"pol_pred{i}"], rtol=0, atol=LOGIT_TOL)
    plan_x = eng.layer_plan()
    kv = eng.forward(*args, thresholds=float(g[f"pol_thr{i}"]), probe_always=True, xprobe=False)
    plan_kv = eng.layer_plan()
    assert np.array_equal(_np(kv.exit_layer), g[f"pol_exits{i}"])
    # the X-space probe projects Q | K | V only for the rows that stay: fewer rows than the K | V probe wherever somebody left
    assert sum(plan_x["rows_qkv"]) <= sum(plan_kv["rows_qkv"]) and (sum(plan_x["rows_qkv"]) < sum(plan_kv["rows_qkv"]) or
                                                                   len(np.unique(g[f"pol_exits{i}"])) == 1)
    eng.close()
    e32 = pkg.EarlyExitEngine(pkg.ModelConfig.tiny(EE_config=dict(exits=[1, 2], encoder_layer_strategy="ramp")), max_docs=2, max_text_len=16)
    assert e32.precision == "fp32" and e32.xprobe_default is False
    e32.close()


def test_one_term_mode_is_a_bounded_deviation(pkg, oracle):
    """MMEE_FLAG_ONE_TERM (the reported low-precision mode: one f16 MFMA term per MAC in the layer GEMMs and the attention) against the
    base-shape golden vectors: it must really differ from the split precision (it is not the parity path), stay a small deviation (hidden
    states carry ~11 significant bits through 12 layers), and flip few exits; the default path on the same handle is untouched by it."""
    g = load_golden("base_cls")
    cfg = pkg.ModelConfig.base(EE_config=BASE_EE)
    W = pkg.synth.make_weights(cfg, seed=int(g["seed_w"]))
    docs = pkg.synth.make_documents(cfg, int(g["n_docs"]), seed=int(g["seed_docs"]), text_len=int(g["text_len"]))
    eng = _engine(pkg, cfg, W, max_docs=4, T=512, precision="split")
    args = (docs["input_ids"], docs["attention_mask"], docs["bbox"], docs["pixel_values"])
    lp = eng.forward(*args, dump_all=True, want_all=True, one_term=True, validate=True)
    full = eng.forward(*args, dump_all=True, want_all=True, validate=True)
    np.testing.assert_allclose(_np(full.all_logits), g["logits_store"], rtol=0, atol=LOGIT_TOL)      # the flag leaves nothing behind
    d = np.abs(_np(lp.all_logits) - g["logits_store"])
    report_measured("one_term[base goldens]", "max|dlogit| vs reference", float(d.max()))
    assert np.isfinite(_np(lp.all_logits)).all()
    assert 1e-5 < d.max() < 0.25 * max(1.0, float(np.abs(g["logits_store"]).max()))
    conf_ref = oracle.softmax64(g["logits_store"]).max(-1)
    conf_lp = oracle.softmax64(_np(lp.all_logits).astype(np.float64)).max(-1)
    report_measured("one_term[base goldens]", "max|d confidence|", float(np.abs(conf_lp - conf_ref).max()))
    assert np.abs(conf_lp - conf_ref).max() < 0.05
    eng.close()


@pytest.mark.gpu
def test_inputs_embeds_vs_oracle_and_vs_input_ids(pkg, oracle):
    """`inputs_embeds` of the reference signature (EE/models/LayoutLMv3.py:383, 414-417; HF:148-158, 171-186) through ee_set_inputs_embeds:
    (1) the word rows of the tokens handed in as inputs_embeds TOGETHER with input_ids reproduce the input_ids call bit for bit (HF takes the
    position ids from input_ids and the rows from inputs_embeds); (2) arbitrary rows WITHOUT input_ids (sequential position ids, nothing is
    padding unless the mask says so) against oracle.forward_all, both precisions, dump-all and early exit; (3) the model mirror's forward."""
    ee = dict(exits=["text_avg", "text_visual_concat", 1, 2], encoder_layer_strategy="ramp")
    from .conftest import H256_KW
    cfg = pkg.ModelConfig.tiny(EE_config=ee, **H256_KW)
    W = pkg.synth.make_weights(cfg, seed=51, head_gain=6.0)
    B, T = 6, 48
    docs = pkg.synth.make_documents(cfg, B, seed=52, text_len=T, min_words=3)
    word = W["layoutlmv3.embeddings.word_embeddings.weight"]
    rng = np.random.default_rng(53)
    free = (word[rng.integers(0, cfg.vocab_size, size=(B, T))] + 0.05 * rng.standard_normal((B, T, cfg.hidden_size))).astype(np.float32)
    for precision in ("fp32", "split"):
        eng = pkg.EarlyExitEngine(cfg, max_docs=B, max_text_len=T, precision=precision, xprobe=False)
        eng.load_weights(W)
        kw = dict(attention_mask=docs["attention_mask"], bbox=docs["bbox"], pixel_values=docs["pixel_values"])
        a = eng.forward(input_ids=docs["input_ids"], **kw, dump_all=True, want_all=True, validate=True)
        b = eng.forward(input_ids=docs["input_ids"], inputs_embeds=word[docs["input_ids"]], **kw, dump_all=True, want_all=True, validate=True)
        assert np.array_equal(_np(a.all_logits), _np(b.all_logits)), precision
        c = eng.forward(input_ids=docs["input_ids"], **kw, dump_all=True, want_all=True, validate=True)      # the setter is consumed by ONE forward
        assert np.array_equal(_np(a.all_logits), _np(c.all_logits)), precision
        batch = dict(inputs_embeds=free, **kw)
        ref = oracle.forward_all(cfg, W, batch, ee["exits"])
        out = eng.forward(inputs_embeds=free, **kw, dump_all=True, want_all=True, validate=True)
        err = float(np.abs(_np(out.all_logits) - ref["logits_store"]).max())
        report_measured(f"inputs_embeds[{precision}]", "max|dlogit|", err)
        assert err < LOGIT_TOL, (precision, err)
        assert np.abs(ref["logits_store"] - oracle.forward_all(cfg, W, docs, ee["exits"])["logits_store"]).max() > 1e-3      # not vacuous
        conf = oracle.softmax64(ref["logits_store"]).max(-1)
        srt = np.sort(conf, axis=1)
        thr = 0.5 * (srt[:, B // 2 - 1] + srt[:, B // 2])
        if np.abs(conf - thr[:, None]).min() >= 1e-5:
            ex, pred, _ = oracle.policy_scan(ref["logits_store"], thr)
            o2 = eng.forward(inputs_embeds=free, **kw, thresholds=thr, validate=True)
            assert np.array_equal(_np(o2.exit_layer), ex), precision
            np.testing.assert_allclose(_np(o2.logits), pred, rtol=0, atol=LOGIT_TOL)
        eng.close()
    model = pkg.LayoutLMv3EEForSequenceClassification(cfg, W, max_docs=4, max_text_len=T)      # 6 documents through a 4-document engine: chunking
    import torch
    res = model(inputs_embeds=torch.from_numpy(free), attention_mask=torch.from_numpy(docs["attention_mask"]), bbox=torch.from_numpy(docs["bbox"]),
                pixel_values=torch.from_numpy(docs["pixel_values"]))
    np.testing.assert_allclose(_np(res.logits), ref["logits_store"][-1], rtol=0, atol=LOGIT_TOL)


@pytest.mark.gpu
def test_output_hidden_states_vs_oracle(pkg, oracle):
    """`output_hidden_states=True` of the reference signature (EE/models/LayoutLMv3.py:164, 182-183, 284-285, 887-896) through
    ee_set_hidden_states_out: the state entering every layer and the last layer's output, every position -- the padded ones included, which the
    reference computes like any other row (dense rows) -- against oracle.forward_all, both precisions; the ragged layout returns the same
    rows and zeros where the mask dropped a position; the logits of the same call are unchanged."""
    ee = dict(exits=["text_avg", 1, 2], encoder_layer_strategy="ramp")
    from .conftest import H256_KW
    cfg = pkg.ModelConfig.tiny(EE_config=ee, **H256_KW)
    W = pkg.synth.make_weights(cfg, seed=61, head_gain=6.0)
    B, T = 5, 48
    docs = pkg.synth.make_documents(cfg, B, seed=62, text_len=T, min_words=3)
    ref = oracle.forward_all(cfg, W, docs, ee["exits"], return_hidden_states=True)
    hs_ref = ref["hidden_states"]
    Pv = (cfg.input_size // cfg.patch_size) ** 2 + 1
    assert hs_ref.shape == (cfg.num_hidden_layers + 1, B, T + Pv, cfg.hidden_size) and (docs["attention_mask"] == 0).any()
    for precision in ("fp32", "split"):
        eng = pkg.EarlyExitEngine(cfg, max_docs=B, max_text_len=T, precision=precision, xprobe=False)
        eng.load_weights(W)
        kw = dict(input_ids=docs["input_ids"], attention_mask=docs["attention_mask"], bbox=docs["bbox"], pixel_values=docs["pixel_values"])
        out = eng.forward(**kw, dump_all=True, want_all=True, want_hidden_states=True, validate=True)
        err = float(np.abs(_np(out.hidden_states) - hs_ref).max())
        report_measured(f"hidden_states[{precision}]", "max|dx|", err)
        assert err < LOGIT_TOL, (precision, err)
        assert float(np.abs(_np(out.all_logits) - ref["logits_store"]).max()) < LOGIT_TOL
        plain = eng.forward(**kw, dump_all=True, want_all=True, validate=True)
        assert float(np.abs(_np(out.all_logits) - _np(plain.all_logits)).max()) < 1e-5      # dense vs ragged rows: same results
        with pytest.raises(ValueError):
            eng.forward(**kw, thresholds=0.5, want_hidden_states=True)
        # the C-ABI's ragged variant: same rows, zeros at dropped positions
        import ctypes as C
        import torch
        hs = torch.full(tuple(hs_ref.shape), float("nan"), dtype=torch.float32, device=eng.device)
        pkg.capi.check(eng.lib.ee_set_hidden_states_out(eng._h, C.c_void_p(hs.data_ptr())), eng._h, "ee_set_hidden_states_out")
        eng.forward(**kw, dump_all=True, whole_layers=True, validate=True)
        got = _np(hs)
        keep = np.concatenate([docs["attention_mask"] != 0, np.ones((B, Pv), dtype=bool)], axis=1)
        assert float(np.abs(got[:, keep] - hs_ref[:, keep]).max()) < LOGIT_TOL and not np.isnan(got).any()
        assert np.all(got[:, ~keep] == 0)
        # a call that fails its validation consumes the one-shot pointer too: the next forward must not write through it
        hs.fill_(7.0)
        pkg.capi.check(eng.lib.ee_set_hidden_states_out(eng._h, C.c_void_p(hs.data_ptr())), eng._h, "ee_set_hidden_states_out")
        with pytest.raises(pkg.capi.MMEEError):
            eng.forward(**kw, thresholds=0.5, whole_layers=True)          # no dump-all: refused by the library
        eng.forward(**kw, dump_all=True, whole_layers=True, validate=True)
        torch.cuda.synchronize()
        assert bool((hs == 7.0).all())
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("H,cs,ss", [(384, 64, 64), (512, 96, 64), (640, 96, 128), (896, 160, 128)])
def test_untested_hidden_sizes_vs_oracle(pkg, oracle, H, cs, ss):
    """The hidden sizes ee_create accepts and no other forward runs: the two-vector row kernels (384, 512) and the masked forms of the three- and
    four-vector ones (640, 896).  Two layers, head dim 64, intermediate 2 H, three ragged documents, every exit kind, dump-all against
    oracle.forward_all; `output_hidden_states` compares EVERY row, not row 0 alone.  f32, and split where the hidden size allows it."""
    ee = dict(exits=["vision_avg", "text_avg", "text_visual_concat", 1, 2], encoder_layer_strategy="ramp")
    cfg = pkg.ModelConfig.tiny(EE_config=ee, hidden_size=H, num_attention_heads=H // 64, intermediate_size=2 * H, num_hidden_layers=2,
                               coordinate_size=cs, shape_size=ss)
    W = pkg.synth.make_weights(cfg, seed=71)
    B, T = 3, 40
    docs = pkg.synth.make_documents(cfg, B, seed=72, text_len=T, min_words=3)
    lengths = (docs["attention_mask"] != 0).sum(1)
    assert len(set(lengths.tolist())) > 1 and (lengths < T).any()                        # ragged
    ref = oracle.forward_all(cfg, W, docs, ee["exits"], return_hidden_cls=True, return_hidden_states=True)
    kw = dict(input_ids=docs["input_ids"], attention_mask=docs["attention_mask"], bbox=docs["bbox"], pixel_values=docs["pixel_values"])
    for precision in ("fp32", "split") if H % 256 == 0 else ("fp32",):
        eng = pkg.EarlyExitEngine(cfg, max_docs=B, max_text_len=T, precision=precision, xprobe=False)
        assert eng.precision == precision
        eng.load_weights(W)
        out = eng.forward(**kw, dump_all=True, want_all=True, want_hidden_cls=True, validate=True)
        for name, got, want, tol in (("hidden_cls", out.hidden_cls, ref["hidden_cls"], 5e-5), ("all_logits", out.all_logits, ref["logits_store"], LOGIT_TOL)):
            err = float(np.abs(_np(got) - want).max())
            report_measured(f"hidden_size[{H},{precision}]", f"max|d {name}|", err)
            assert err <= tol, (name, precision, err)
        hs = eng.forward(**kw, dump_all=True, want_all=True, want_hidden_states=True, validate=True)
        err = float(np.abs(_np(hs.hidden_states) - ref["hidden_states"]).max())
        report_measured(f"hidden_size[{H},{precision}]", "max|d hidden_states|, every row", err)
        assert err < LOGIT_TOL, (precision, err)
        eng.close()
    if H % 256:
        with pytest.raises(pkg.capi.MMEEError, match="multiples of 256"):
            pkg.EarlyExitEngine(cfg, max_docs=B, max_text_len=T, precision="split", xprobe=False)
