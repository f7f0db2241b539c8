"""The float64 restatement of the row kernels (tests/rows_ref.py), checked without a GPU: it agrees with the oracle's embeddings, LayerNorm,
position ids and visual boxes, its inputs are what its header promises, and they can SEE a subtly wrong kernel -- every mutation below moves a
checked output by at least 10 times the tolerance that output's row is held to in tests/test_gpu_rows.py (integer outputs: they differ)."""
import types

import numpy as np
import pytest

from . import rows_ref as R

CONFIGS = [(128, 24, 16), (640, 96, 128), (1024, 171, 170)]


@pytest.fixture(scope="module", params=CONFIGS, ids=lambda c: f"H{c[0]}_cs{c[1]}")
def emb(request):
    c = R.EmbedCase(*request.param, type_vocab=2)
    ref = R.embed_ref(c)
    y = R.embed_f32_torch(c)
    tol = {k: R.tolerance(R.per_row_max(y[k].astype(np.float64) - ref[k])) for k in ("X", "text", "vis", "cat")}
    return c, ref, tol


def _oracle_view(c):
    """The case as the oracle's (cfg, W, pixel_values): a 1 x 1 patch projection with the identity as its weight hands vis_raw through exactly."""
    cfg = types.SimpleNamespace(pad_token_id=R.PAD, max_2d_position_embeddings=R.MAX_2D, layer_norm_eps=R.EPS, hidden_size=c.H, patch_size=1, input_size=c.G)
    p, e = "layoutlmv3.", "layoutlmv3.embeddings."
    W = {e + "word_embeddings.weight": c.word, e + "token_type_embeddings.weight": c.type, e + "position_embeddings.weight": c.pos,
         e + "x_position_embeddings.weight": c.xtab, e + "y_position_embeddings.weight": c.ytab, e + "h_position_embeddings.weight": c.htab,
         e + "w_position_embeddings.weight": c.wtab, e + "LayerNorm.weight": c.text_g, e + "LayerNorm.bias": c.text_b,
         p + "patch_embed.proj.weight": np.eye(c.H, dtype=np.float32).reshape(c.H, c.H, 1, 1), p + "patch_embed.proj.bias": np.zeros(c.H, np.float32),
         p + "cls_token": c.cls_token, p + "pos_embed": c.pos_embed, p + "norm.weight": c.vis_g, p + "norm.bias": c.vis_b}
    pix = c.vis_raw.reshape(c.B, c.G, c.G, c.H).transpose(0, 3, 1, 2)
    return cfg, W, pix


# a float32 LayerNorm of rows of magnitude <= 4: a few 1e-7 per operation, 4e-6 (one ulp of 50 deviations) on the large-mean rows
F32_ACCURACY = 1e-5


def test_the_restatement_agrees_with_the_oracle(emb, oracle):
    c, ref, _ = emb
    cfg, W, pix = _oracle_view(c)
    lay = ref["lay"]
    assert np.array_equal(R.position_ids(c.ids, R.PAD), oracle.position_ids_from_input_ids(c.ids, R.PAD))
    assert np.array_equal(lay["emb_pos"], oracle.position_ids_from_input_ids(c.ids, R.PAD))
    for G in (2, 6, 14):
        vb = oracle.visual_bbox(G)
        x0, y1 = R.visual_boxes(G)
        assert np.array_equal(x0, vb[:, 0]) and np.array_equal(y1, vb[:, 3])
    for embeds in (False, True):
        r = R.embed_ref(c, use_embeds=embeds)
        t1 = oracle.text_embeddings(cfg, W, c.ids, c.bbox, c.tt, None, c.inputs_embeds if embeds else None)
        v1 = oracle.image_embeddings(cfg, W, pix)
        x = oracle.layer_norm(np.concatenate([t1, v1], 1), c.ln2_g, c.ln2_b, R.EPS)
        packed = np.concatenate([np.concatenate([x[b, :c.T][lay["text_dst"][b] >= 0], x[b, c.T:]]) for b in range(c.B)])
        for name, got, want in (("rows", packed, r["X"]), ("text_avg", t1.mean(1), r["text"]), ("vision_avg", v1.mean(1), r["vis"]),
                                ("text_visual_concat", x.mean(1), r["cat"])):
            err = np.abs(got - want).max()
            print(f"{name}, inputs_embeds {embeds}: max |oracle - ref64| = {err:.2e}")
            assert err < F32_ACCURACY, (name, err)
    y = R.layer_norm(c.vis_raw[0], c.vis_g, c.vis_b, R.VIS_EPS)
    assert np.abs(oracle.layer_norm(c.vis_raw[0], c.vis_g, c.vis_b, R.VIS_EPS) - y).max() < F32_ACCURACY


def test_the_embedding_case_is_the_one_the_kernel_tests_describe(emb):
    c, ref, tol = emb
    lay = ref["lay"]
    assert (c.B, c.T, c.Pv) == (2, 41, 37) and 4 * c.cs + 2 * c.ss == c.H
    assert lay["ntext"].tolist() == [30, 38] and lay["n_rows"] == 30 + 38 + 2 * 37          # trailing pads dropped, the hole stays a row
    assert lay["text_dst"][1, 17] == 17 and c.mask[1, 17] == 0 and lay["meta"][67 + 17, 3] == R.KEY_MASKED
    for a in (c.word, c.type, c.pos, c.xtab, c.ytab, c.htab, c.wtab, c.cls_token, c.pos_embed, c.vis_raw, c.inputs_embeds):
        assert a.dtype == np.float32 and np.array_equal(np.round(a / R.GRID) * R.GRID, a) and np.abs(a).max() < 4           # exact row sums
    big = c.word[R.VOCAB - R.N_LARGE:]
    assert (np.abs(big.mean(-1) / big.std(-1)) > 40).all() and np.isin(c.ids, np.arange(R.VOCAB - R.N_LARGE, R.VOCAB)).sum() >= 4
    assert ((c.bbox[..., 2] < c.bbox[..., 0]) & (c.mask != 0)).sum() >= 10 and ((c.bbox[..., 3] < c.bbox[..., 1]) & (c.mask != 0)).sum() >= 10
    assert all(np.isfinite(ref[k]).all() for k in ("X", "text", "vis", "cat"))
    print("tolerance per row, max:", {k: f"{v.max():.2e}" for k, v in tol.items()})
    assert max(v.max() for v in tol.values()) < 2 * F32_ACCURACY


EMBED_MUTATIONS = {                     # name -> the float outputs it must move
    "eps_swapped": ("X", "vis", "cat"), "var_h_minus_1": ("X", "text", "vis", "cat"), "one_pass_var_f32": ("X",), "hw_swapped": ("X", "text", "cat"),
    "height_from_x": ("X", "text", "cat"), "no_clip": ("X", "text", "cat"), "posid_no_mask_factor": ("X", "text", "cat"),
    "posid_start_at_pad": ("X", "text", "cat"), "pool_kept_only": ("text", "cat"), "pool_div_kept": ("text", "cat"),
}
MARGIN = 10.0


@pytest.mark.parametrize("mut", list(EMBED_MUTATIONS))
def test_the_embedding_case_sees_a_subtle_fault(emb, mut):
    c, ref, tol = emb
    other = R.embed_ref(c, mut=mut)
    for k in EMBED_MUTATIONS[mut]:
        ratio = float((R.per_row_max(other[k] - ref[k]) / tol[k]).max())
        print(f"H={c.H} {mut}: {k} moves by {ratio:.1f} x its tolerance")
        assert ratio >= MARGIN, (mut, k, ratio)


@pytest.mark.parametrize("mut,fields", [("y1_from_bbox1", ("meta",)), ("posid_no_mask_factor", ("emb_pos",)), ("posid_start_at_pad", ("emb_pos",)),
                                        ("hole_dropped", ("text_dst", "ntext", "doc_off", "meta")),
                                        ("trailing_pads_kept", ("text_dst", "ntext", "doc_off", "meta"))])
def test_the_prep_cases_see_a_subtle_fault(mut, fields):
    """Integer outputs are held to equality: the mutation must change them, on the embedding case and on the prep tests' own inputs."""
    c = R.EmbedCase(128, 24, 16)
    for f in fields:
        assert not np.array_equal(c.prep(mut=mut)[f], c.prep()[f]), f
    kind = "hole" if mut in ("hole_dropped", "posid_no_mask_factor") else "trailing"
    for T in (9, 33, 257):
        ids, am, bbox = R.make_prep_inputs(3, T, kind)
        a, b = (R.prep_ref(ids, am, bbox, 2, max_pos=T + 2, mut=m) for m in ("", mut))
        for f in fields:
            assert not np.array_equal(a[f], b[f]), (T, f)


def test_prep_inputs_are_what_the_masks_say():
    for T in (1, 8, 9, 33, 257, 512):
        for kind in R.MASKS:
            ids, am, bbox = R.make_prep_inputs(3, T, kind)
            p = R.prep_ref(ids, am, bbox, 2, max_pos=T + 2)
            assert p["err"] == 0 and (p["ntext"] >= 1).all() and p["doc_off"][-1] == p["n_rows"] == p["ntext"].sum() + 3 * 5
            if kind in ("full", "null", "last_only"):
                assert (p["ntext"] == T).all()
            if kind == "zero":
                assert (p["ntext"] == 1).all() and (p["meta"][p["doc_off"][:-1], 3] == R.KEY_MASKED).all()
            if kind == "trailing" and T >= 8:
                assert len(set(p["ntext"].tolist())) > 1 and (p["ntext"] < T).any()
            if kind == "hole" and T >= 8:
                inside = [(am[b, :p["ntext"][b]] == 0).sum() for b in range(3)]
                assert min(inside) >= 1
            assert np.array_equal(R.prep_ref(ids, am, bbox, 2, max_pos=T + 2, dense_rows=True)["ntext"], [T] * 3)


LN_MUTATIONS = ("var_h_minus_1", "one_pass_var_f32", "drop_last_part", "resid_not_gathered", "resid_inv_x2")


@pytest.mark.parametrize("parts", [2, 4])
@pytest.mark.parametrize("H", [128, 384, 1024])
def test_the_layernorm_case_sees_a_subtle_fault(H, parts):
    c = R.LnCase(H, 5, pre_parts=parts)
    ref = R.ln_rows_ref(c)
    tol = R.tolerance(R.per_row_max(R.ln_rows_f32_torch(c).astype(np.float64) - ref))
    assert np.array_equal(R.split_round(c.resid, R.SPLIT_SCALE), c.resid.astype(np.float64))          # the planes hold the residual exactly
    norms = np.sqrt((c.parts[:, c.rows(3)].astype(np.float64) ** 2).sum(-1))
    assert norms[-1] > 0.3 * norms[0]                                                                 # a last part comparable to the first
    assert c.const_ok and np.array_equal(ref[R.CONST_ROW], c.b.astype(np.float64))                    # the constant row: beta exactly
    big = c.parts[:, c.rows(1)].astype(np.float64).sum(0) + c.bias + c.resid[c.resid_rows[1]]
    assert abs(big.mean() / big.std()) > 40
    print(f"H={H} parts={parts}: tolerance per row {tol}")
    assert tol.max() < 2e-5
    for mut in LN_MUTATIONS:
        ratio = float((R.per_row_max(R.ln_rows_ref(c, mut) - ref) / tol).max())
        print(f"H={H} parts={parts} {mut}: moves a row by {ratio:.1f} x its tolerance")
        assert ratio >= MARGIN, (mut, ratio)
