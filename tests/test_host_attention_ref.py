"""The float64 attention reference of the kernel tests (tests/attn_ref.py), checked without a GPU: it agrees with the oracle's encoder layer, the
plane emulation is exact, and the shared ragged batch can SEE a subtly wrong kernel -- every mutation below moves a document's context by at least
100 times the tolerance that document is held to in tests/test_gpu_attention.py."""
import math

import numpy as np
import pytest

from . import attn_ref as R


@pytest.fixture(scope="module", params=[3, 2], ids=["heads3", "heads2"])
def case(request):
    b = R.make_batch(heads=request.param)
    ref = R.attention_ref(b)
    err32 = R.per_doc_max(b, R.attention_f32_torch(b).astype(np.float64) - ref)
    return b, ref, err32


def test_the_ragged_batch_is_the_one_the_kernel_tests_describe(case):
    b, ref, err32 = case
    assert tuple(b.lengths) == R.RAGGED_LENGTHS and b.n_docs == 19 and b.lengths.max() == 257
    assert np.array_equal(R.split_round(b.qkv, R.SCALE_QKV), b.qkv.astype(np.float64))          # pre-rounded: a second split changes nothing
    for d, L in enumerate(b.lengths):
        m = b.masked[b.rows(d)]
        assert m[0] == 0 and m.sum() == (L // 6 if L >= 33 else 0)
    assert np.isfinite(ref).all()
    print("float32 yardstick, max |err32| per document:", ", ".join(f"L={L}: {e:.2e}" for L, e in zip(b.lengths, err32)))
    assert err32.max() < 2e-5                       # a float32 attention of these sizes: a few 1e-6


def test_split_round_is_the_plane_arithmetic():
    rng = np.random.default_rng(3)
    x = np.concatenate([rng.standard_normal(4096) * 3, [0.0, 1.0, -1.0, 2.0 ** -12, 60.0 + 2.0 ** -6, 1e-4]]).astype(np.float32)
    for s in (16.0, 64.0, 1024.0):
        y = R.split_round(x, s)
        # hi + lo carries 22 significant bits; a lo plane in the f16 subnormal range steps by 2^-24
        assert (np.abs(y - x.astype(np.float64)) <= np.abs(x) * 2.0 ** -21 + 2.0 ** -25 / s).all()
        assert np.array_equal(R.split_round(y, s), y)                                           # idempotent
    assert R.split_round(np.float32(1.0 + 2.0 ** -12), 16.0) == 1.0 + 2.0 ** -12                # kept by the lo plane
    lost = np.float32(1.0 + 2.0 ** -11 + 2.0 ** -23)                                            # the remainder of hi needs 12 bits: lo rounds
    assert R.split_round(lost, 16.0) != float(lost) and abs(R.split_round(lost, 16.0) - float(lost)) <= 2.0 ** -22


def _moved(b, ref, other):
    return R.per_doc_max(b, other - ref)


def test_every_document_can_see_a_subtle_fault(case):
    """Mutations of the REFERENCE, each against the tolerance max(FACTOR * err32, 1e-6) of the document: (1) the last unmasked key dropped,
    (2) one masked key unmasked, (3) one (query, key) pair per row in the neighbouring 1-D bucket, (4) the V rows of the last two unmasked keys
    swapped.  (1) and (3) need a second unmasked key -- a softmax over one key is 1 whatever happens to its score -- so the one-row document
    takes part in none; (2) needs a masked key, (4) two rows."""
    b, ref, err32 = case
    tol = R.tolerance(err32)
    H = b.qkv.shape[1] // 3
    live = [np.nonzero(b.masked[b.rows(d)] == 0)[0] for d in range(b.n_docs)]
    dead = [np.nonzero(b.masked[b.rows(d)] != 0)[0] for d in range(b.n_docs)]
    ratios = {}

    m = b.copy()
    for d in range(b.n_docs):
        if len(live[d]) >= 2:
            m.masked[b.doc_off[d] + live[d][-1]] = 1
    ratios["last key dropped"] = (_moved(b, ref, R.attention_ref(m)) / tol, [d for d in range(b.n_docs) if len(live[d]) >= 2])

    m = b.copy()
    for d in range(b.n_docs):
        if len(dead[d]):
            m.masked[b.doc_off[d] + dead[d][len(dead[d]) // 2]] = 0
    ratios["masked key unmasked"] = (_moved(b, ref, R.attention_ref(m)) / tol, [d for d in range(b.n_docs) if len(dead[d])])

    def neighbour(d, b1):
        b1 = b1.copy()
        L = b1.shape[0]
        k = live[d][(np.arange(L) * 7 + 3) % len(live[d])]          # a different unmasked key for every query row
        k = np.where(k == np.arange(L), live[d][(np.arange(L) * 7 + 4) % len(live[d])], k) if len(live[d]) >= 2 else k
        q = np.arange(L)
        b1[q, k] = np.where(b1[q, k] + 1 < b.w1.shape[1], b1[q, k] + 1, b1[q, k] - 1)
        return b1
    ratios["neighbouring 1-D bucket"] = (_moved(b, ref, R.attention_ref(b, b1_hook=neighbour)) / tol,
                                         [d for d in range(b.n_docs) if len(live[d]) >= 2])

    m = b.copy()
    for d in range(b.n_docs):
        if len(live[d]) >= 2:
            i, j = b.doc_off[d] + live[d][-2], b.doc_off[d] + live[d][-1]
            m.qkv[[i, j], 2 * H:] = b.qkv[[j, i], 2 * H:]
    ratios["V rows swapped"] = (_moved(b, ref, R.attention_ref(m)) / tol, [d for d in range(b.n_docs) if b.lengths[d] >= 2])

    for name, (r, docs) in ratios.items():
        assert docs, name
        k = min(docs, key=lambda d: r[d])
        print(f"sensitivity[heads={b.heads}] {name}: smallest ratio {r[k]:.0f} at length {b.lengths[k]} ({len(docs)} documents)")
        assert min(r[d] for d in docs) >= 100.0, (name, [(int(b.lengths[d]), float(r[d])) for d in docs if r[d] < 100.0])


def test_the_reference_is_the_oracles_attention(pkg, oracle):
    """attn_ref against oracle.encoder_layer on a tiny config, so the new reference is not a second opinion of our own: the scores the layer
    forms (HF:263-272) and the probabilities it returns (`probs_out`), for padded documents with masked keys."""
    cfg = pkg.ModelConfig.tiny(EE_config=dict(exits=[1], encoder_layer_strategy="ramp"))
    W = pkg.synth.make_weights(cfg, seed=3)
    docs = pkg.synth.make_documents(cfg, 3, seed=4, text_len=24, min_words=5)
    B, T = docs["input_ids"].shape
    nh, H = cfg.num_attention_heads, cfg.hidden_size
    d = H // nh
    g = cfg.input_size // cfg.patch_size
    am = docs["attention_mask"].copy()
    am[0, 2] = 0                                        # a hole
    x = np.concatenate([oracle.text_embeddings(cfg, W, docs["input_ids"], docs["bbox"]), oracle.image_embeddings(cfg, W, docs["pixel_values"])], axis=1)
    S = x.shape[1]
    pos = np.concatenate([np.broadcast_to(np.arange(T), (B, T)), np.broadcast_to(np.arange(S - T), (B, S - T))], axis=1)
    bbox = np.concatenate([docs["bbox"], np.broadcast_to(oracle.visual_bbox(g), (B, S - T, 4))], axis=1)
    keymask = np.concatenate([am, np.ones((B, S - T), np.int64)], axis=1)
    bias = oracle.attention_bias(cfg, W, pos, bbox)
    ext = ((1.0 - keymask[:, None, None, :].astype(np.float32)) * np.finfo(np.float32).min).astype(np.float32)
    probs = []
    oracle.encoder_layer(cfg, W, 0, x, bias, ext, probs_out=probs)
    q = "layoutlmv3.encoder.layer.0.attention.self."
    lin = lambda n: oracle.linear(x, W[q + n + ".weight"], W[q + n + ".bias"])
    Q, K, V = lin("query") / np.float32(math.sqrt(d)), lin("key"), lin("value")
    e = "layoutlmv3.encoder."
    b = R.Batch(np.concatenate([Q, K, V], axis=-1).reshape(B * S, 3 * H).astype(np.float32), np.arange(B + 1) * S, pos.reshape(-1).astype(np.int32),
                bbox[..., 0].reshape(-1).astype(np.int32), bbox[..., 3].reshape(-1).astype(np.int32), (1 - keymask).reshape(-1).astype(np.int32),
                W[e + "rel_pos_bias.weight"], W[e + "rel_pos_x_bias.weight"], W[e + "rel_pos_y_bias.weight"], nh)
    assert (cfg.rel_pos_bins, cfg.rel_2d_pos_bins, cfg.max_rel_pos, cfg.max_rel_2d_pos) == (R.BINS[0], R.BINS[1], R.MAX_REL_POS, R.MAX_REL_2D_POS)
    heads = lambda t: t.reshape(B, S, nh, d).transpose(0, 2, 1, 3)
    s_oracle = heads(Q).astype(np.float64) @ heads(K).astype(np.float64).transpose(0, 1, 3, 2) + bias.astype(np.float64) / math.sqrt(d)
    for i in range(B):
        s, p, ctx = R.attention_doc(b, i)
        live = keymask[i] != 0
        assert np.isneginf(s[:, :, ~live]).all()
        err_s = np.abs(s[:, :, live] - s_oracle[i][:, :, live]).max()
        err_p = np.abs(p - probs[0][i].astype(np.float64)).max()
        print(f"attn_ref vs oracle, document {i}: max |d score| {err_s:.2e}, max |d probability| {err_p:.2e}")
        assert err_s <= 2e-6 and err_p <= 1e-6          # the oracle's bias and probabilities are float32
        ctx32 = R.attention_f32_torch(b.select([i]))
        assert np.abs(ctx32 - ctx).max() <= 1e-5
