"""What the thirteen stand-alone kernel hooks (ee_debug_attention, ee_debug_xprobe, ee_debug_prep, ee_debug_embed, ee_debug_ln_rows,
ee_debug_head_out, ee_debug_exit_decide, ee_debug_rows_out, ee_debug_patch_project, ee_debug_gemm_routes, ee_debug_gemm_f32, ee_debug_split_rows,
ee_debug_split_weight) refuse before they ask for a device: every refusal below is decided on the host from the arguments alone, so the message is asserted whole, on a machine
without a GPU too.  The pointers are fake and never dereferenced: every call in this file is refused first."""
import ctypes as C

P = C.c_void_p(4096)


def _refused(pkg, who, rc, text, what):
    msg = pkg.capi.last_error()
    assert rc != 0, (who, what)
    assert msg == f"{who}: {text}", (what, msg)


def test_attention_refusals(pkg):
    lib, who = pkg.capi.load(), "ee_debug_attention"
    err = C.c_int32(-1)

    def call(**over):
        a = dict(qkv=P, qkv_rows=100, doc_off=P, n_docs=2, qkv_doc_off=None, pos=P, x0=P, y1=P, masked=P, w1=P, wx=P, wy=P, heads=2, bins1=32, bins2=64,
                 max_rel_pos=128, max_rel_2d_pos=256, max_pos=300, max_coord=1000, kernel=2, use_queue=1, q_limit=0, terms=3, ctx=P,
                 err=C.byref(err))
        a.update(over)
        return lib.ee_debug_attention(*a.values(), None)

    bad = "bad argument (pointers not NULL, n_docs >= 1, 1 <= heads <= 64, q_limit >= 0, max_pos <= 4095, max_coord <= 65535)"
    bias = "the bias needs w1 / wx / wy, 4 <= bins <= 256 and max_rel_pos, max_rel_2d_pos >= 1"
    terms = "terms is 3, or 1 for MMEE_ATTN_KERNEL_IDX (the one-term mode is built for that kernel only)"
    f32 = "attention_f32 takes neither q_limit nor qkv_doc_off (probe-first layers are split-precision)"
    cases = [
        (dict(kernel=4), "kernel 4 is none of MMEE_ATTN_KERNEL_F32, _PAIR, _IDX, _IDX_NOBIAS"),
        (dict(kernel=-1), "kernel -1 is none of MMEE_ATTN_KERNEL_F32, _PAIR, _IDX, _IDX_NOBIAS"),
        (dict(kernel=4, qkv=None), "kernel 4 is none of MMEE_ATTN_KERNEL_F32, _PAIR, _IDX, _IDX_NOBIAS"),      # the kernel id is looked at first
        (dict(qkv=None), bad), (dict(doc_off=None), bad), (dict(pos=None), bad), (dict(x0=None), bad), (dict(y1=None), bad), (dict(masked=None), bad),
        (dict(ctx=None), bad), (dict(err=None), bad), (dict(n_docs=0), bad), (dict(heads=0), bad), (dict(heads=65), bad), (dict(qkv_rows=0), bad),
        (dict(q_limit=-1), bad), (dict(max_pos=-1), bad), (dict(max_pos=4096), bad), (dict(max_coord=-1), bad), (dict(max_coord=65536), bad),
        (dict(kernel=3, masked=None), bad),                                     # the image-only form too
        (dict(w1=None), bias), (dict(kernel=0, wx=None), bias), (dict(kernel=1, wy=None), bias), (dict(bins1=3), bias), (dict(bins1=257), bias),
        (dict(bins2=3), bias), (dict(bins2=257), bias), (dict(max_rel_pos=0), bias), (dict(max_rel_2d_pos=0), bias),
        (dict(w1=None, terms=2), bias),                                         # the bias operands before terms
        (dict(terms=2), terms), (dict(terms=0), terms), (dict(kernel=1, terms=1), terms), (dict(kernel=0, terms=1), terms),
        (dict(kernel=3, terms=1, w1=None, wx=None, wy=None), terms),            # the image-only form needs no bias operands, and has no one-term mode
        (dict(kernel=0, q_limit=32), f32), (dict(kernel=0, qkv_doc_off=P), f32),
    ]
    for over, text in cases:
        _refused(pkg, who, call(**over), text, over)


def _xprobe_args(pkg, **over):
    a = pkg.capi.DebugXProbeArgs()
    for name, kind in a._fields_:
        if kind is C.c_void_p:
            setattr(a, name, 4096)
    vals = dict(n_orig=3, n_docs=2, max_docs=4, x_rows=100, ctx_rows=100, H=768, heads=12, bins1=32, bins2=64, max_rel_pos=128, max_rel_2d_pos=256,
                max_pos=300, max_coord=1000, index_form=0, cus=0)
    vals.update(over)
    for k, v in vals.items():
        setattr(a, k, v)
    return a


def test_xprobe_refusals(pkg):
    lib, who = pkg.capi.load(), "ee_debug_xprobe"
    err = C.c_int32(-1)
    call = lambda **over: lib.ee_debug_xprobe(C.byref(_xprobe_args(pkg, **over)), C.byref(err), None)
    _refused(pkg, who, lib.ee_debug_xprobe(None, C.byref(err), None), "args and err_flag_out must not be NULL", "args")
    _refused(pkg, who, lib.ee_debug_xprobe(C.byref(_xprobe_args(pkg)), None, None), "args and err_flag_out must not be NULL", "err_flag_out")
    null = "an input pointer or ctx is NULL (only u_out, s0_out, cvec_out and order_out may be)"
    counts = "bad counts (n_orig >= 1, 0 <= n_docs <= max_docs, 1 <= max_docs <= 2^20, x_rows >= 1, ctx_rows >= 1)"
    bins = "the bias needs 4 <= bins <= 256, max_rel_pos, max_rel_2d_pos >= 1, max_pos <= 4095, max_coord <= 65535"
    cases = [(dict([(k, None)]), null) for k in ("orig_doc_off", "pos", "x0", "y1", "masked", "doc_off", "doc_orig", "x_phys", "xs", "qc", "wk", "bk", "bv", "wv",
                                                  "w1", "wx", "wy", "ctx")]
    cases += [
        (dict(wk=None, n_orig=0), null),                                        # the pointers before the counts
        (dict(n_orig=0), counts), (dict(n_docs=-1), counts), (dict(max_docs=0, n_docs=0), counts), (dict(n_docs=5), counts),
        (dict(max_docs=(1 << 20) + 1), counts), (dict(x_rows=0), counts), (dict(ctx_rows=0), counts),
        (dict(H=32), "hidden size 32 outside [64, 4096] or 12 heads outside [1, 64]"),
        (dict(H=4160), "hidden size 4160 outside [64, 4096] or 12 heads outside [1, 64]"),
        (dict(heads=0), "hidden size 768 outside [64, 4096] or 0 heads outside [1, 64]"),
        (dict(heads=65), "hidden size 768 outside [64, 4096] or 65 heads outside [1, 64]"),
        (dict(bins1=3), bins), (dict(bins1=257), bins), (dict(bins2=3), bins), (dict(bins2=257), bins), (dict(max_rel_pos=0), bins),
        (dict(max_rel_2d_pos=0), bins), (dict(max_pos=-1), bins), (dict(max_pos=4096), bins), (dict(max_coord=-1), bins), (dict(max_coord=65536), bins),
        (dict(index_form=2), "index_form 2 is neither 0 (32-bit pair index) nor 1 (query block 0 of the 16-bit form)"),
        (dict(index_form=-1), "index_form -1 is neither 0 (32-bit pair index) nor 1 (query block 0 of the 16-bit form)"),
        (dict(cus=-1), "cus -1 outside [0, 4096] (0: the device's count)"), (dict(cus=4097), "cus 4097 outside [0, 4096] (0: the device's count)"),
        (dict(index_form=2, cus=-1), "index_form 2 is neither 0 (32-bit pair index) nor 1 (query block 0 of the 16-bit form)"),
    ]
    for over, text in cases:
        _refused(pkg, who, call(**over), text, over)


# what check_prep says for ee_debug_prep and ee_debug_embed alike: (changed arguments, text)
PREP_CASES = [
    (dict(input_ids=None), "input_ids and bbox must not be NULL"), (dict(bbox=None), "input_ids and bbox must not be NULL"),
    (dict(B=0), "bad shape (B >= 1, T >= 1, 1 <= G <= 64, B (T + G G + 1) <= 2^30), got B 0, T 8, G 2"),
    (dict(T=0), "bad shape (B >= 1, T >= 1, 1 <= G <= 64, B (T + G G + 1) <= 2^30), got B 2, T 0, G 2"),
    (dict(G=0), "bad shape (B >= 1, T >= 1, 1 <= G <= 64, B (T + G G + 1) <= 2^30), got B 2, T 8, G 0"),
    (dict(G=65), "bad shape (B >= 1, T >= 1, 1 <= G <= 64, B (T + G G + 1) <= 2^30), got B 2, T 8, G 65"),
    (dict(B=1 << 20, T=1 << 10), "bad shape (B >= 1, T >= 1, 1 <= G <= 64, B (T + G G + 1) <= 2^30), got B 1048576, T 1024, G 2"),
] + [(over, "bad range limits (vocab, max_2d, max_pos, type_vocab >= 1, 0 <= pad_id < max_pos)")
     for over in (dict(vocab=0), dict(max_2d=0), dict(max_pos=0), dict(type_vocab=0), dict(pad_id=-1), dict(pad_id=10))]
PREP_VALUES = dict(B=2, T=8, G=2, pad_id=1, vocab=100, max_2d=1024, max_pos=10, type_vocab=1, dense_rows=0)


def test_prep_refusals(pkg):
    lib, who = pkg.capi.load(), "ee_debug_prep"
    err = C.c_int32(-1)
    outputs = ("text_dst", "emb_pos", "ntext", "doc_off", "x_src", "doc_orig", "meta", "counts")

    def call(**over):
        a = dict(input_ids=P, attention_mask=P, bbox=P, position_ids=None, token_type_ids=None, **PREP_VALUES)
        a.update({k: P for k in outputs}, err=C.byref(err))
        a.update(over)
        return lib.ee_debug_prep(*a.values(), None)

    cases = PREP_CASES + [(dict([(k, None)]), "every output pointer must be given") for k in outputs + ("err",)]
    cases.append((dict(bbox=None, meta=None), "input_ids and bbox must not be NULL"))       # the inputs before the outputs
    for over, text in cases:
        _refused(pkg, who, call(**over), text, over)


def _embed_args(pkg, **over):
    a = pkg.capi.DebugEmbedArgs()
    optional = ("position_ids", "token_type_ids", "inputs_embeds", "Xs", "text_part", "vis_part", "cat_part", "pooled_text", "pooled_vis", "pooled_cat")
    for name, kind in a._fields_:
        if kind is C.c_void_p and name not in optional:
            setattr(a, name, 4096)
    vals = dict(PREP_VALUES, H=128, cs=24, ss=16, text_eps=1e-5, vis_eps=1e-6, eps2=1e-5, split_scale=0.0)
    vals.update(over)
    for k, v in vals.items():
        setattr(a, k, v)
    return a


def test_embed_refusals(pkg):
    lib, who = pkg.capi.load(), "ee_debug_embed"
    err = C.c_int32(-1)
    call = lambda **over: lib.ee_debug_embed(C.byref(_embed_args(pkg, **over)), C.byref(err), None)
    _refused(pkg, who, lib.ee_debug_embed(None, C.byref(err), None), "args and err_flag_out must not be NULL", "args")
    _refused(pkg, who, lib.ee_debug_embed(C.byref(_embed_args(pkg)), None, None), "args and err_flag_out must not be NULL", "err_flag_out")
    table = "a table, LayerNorm vector or visual input is NULL (word may be NULL with inputs_embeds)"
    one = "exactly one of X and Xs receives the rows"
    pair = "a partial-sum buffer and its pooled output are given together or not at all"
    split = dict(X=None, Xs=4096, H=256, cs=48, ss=32, split_scale=16.0)
    cases = list(PREP_CASES) + [
        (dict(H=192, cs=32, ss=32), "hidden size 192 is not a multiple of 128 in [128, 1024]"),
        (dict(H=1152, cs=192, ss=192), "hidden size 1152 is not a multiple of 128 in [128, 1024]"),
        (dict(H=0), "hidden size 0 is not a multiple of 128 in [128, 1024]"),
        (dict(B=0, H=192), "bad shape (B >= 1, T >= 1, 1 <= G <= 64, B (T + G G + 1) <= 2^30), got B 0, T 8, G 2"),      # check_prep before check_hidden
        (dict(cs=25), "4 coordinate_size + 2 shape_size = 132 is not the hidden size 128"),
        (dict(cs=0, ss=64), "4 coordinate_size + 2 shape_size = 128 is not the hidden size 128"),        # the sum is right, a size is not
        (dict(cs=32, ss=0), "4 coordinate_size + 2 shape_size = 128 is not the hidden size 128"),
    ]
    cases += [(dict([(k, None)]), table) for k in ("type", "pos", "xtab", "ytab", "htab", "wtab", "text_ln_g", "text_ln_b", "vis_ln_g", "vis_ln_b", "ln2_g",
                                                   "ln2_b", "cls_token", "pos_embed", "vis_raw", "word")]
    cases += [
        (dict(Xs=4096), one), (dict(X=None), one),
        (dict(X=None, Xs=4096, split_scale=16.0), "split rows need a hidden size that is a multiple of 256 (got 128)"),
        (dict(split, H=384, cs=64, ss=64), "split rows need a hidden size that is a multiple of 256 (got 384)"),
        (dict(split, split_scale=0.0), "split_scale must be positive"), (dict(split, split_scale=-1.0), "split_scale must be positive"),
        (dict(split, split_scale=float("nan")), "split_scale must be positive"),
        (dict(text_part=4096), pair), (dict(pooled_text=4096), pair), (dict(vis_part=4096), pair), (dict(pooled_vis=4096), pair),
        (dict(cat_part=4096), pair), (dict(pooled_cat=4096), pair),
    ]
    for over, text in cases:
        _refused(pkg, who, call(**over), text, over)


def test_ln_rows_refusals(pkg):
    lib, who = pkg.capi.load(), "ee_debug_ln_rows"
    err = C.c_int32(-1)

    def call(**over):
        a = dict(src=P, dst=P, row_src=None, n_rows=P, max_rows=5, H=256, gamma=P, beta=P, eps=1e-5, dst_split=None, split_scale=0.0, pre_parts=0,
                 pre_stride=0, pre_bias=None, pre_resid=None, pre_resid_rows=None, pre_resid_inv=0.0, err=C.byref(err))
        a.update(over)
        return lib.ee_debug_ln_rows(*a.values(), None)

    null = "src, n_rows, gamma, beta, err_flag_out must not be NULL, max_rows >= 0"
    need = "a bias or residual needs pre_parts >= 1"
    cases = [
        (dict(src=None), null), (dict(n_rows=None), null), (dict(gamma=None), null), (dict(beta=None), null), (dict(err=None), null), (dict(max_rows=-1), null),
        (dict(H=192), "hidden size 192 is not a multiple of 128 in [128, 1024]"), (dict(H=1152), "hidden size 1152 is not a multiple of 128 in [128, 1024]"),
        (dict(src=None, H=192), null),                                          # in the order of the entry point
        (dict(dst=None), "neither dst nor dst_split is given"),
        (dict(H=384, dst_split=P, split_scale=16.0), "split rows need a hidden size that is a multiple of 256 (got 384)"),
        (dict(dst=None, dst_split=P, H=128, split_scale=16.0), "split rows need a hidden size that is a multiple of 256 (got 128)"),
        (dict(dst_split=P), "split_scale must be positive"), (dict(dst_split=P, split_scale=-16.0), "split_scale must be positive"),
        (dict(pre_parts=-1), "pre_parts -1 outside [0, 8]"), (dict(pre_parts=9), "pre_parts 9 outside [0, 8]"),
        (dict(pre_bias=P), need), (dict(pre_resid=P), need), (dict(pre_resid_rows=P), need),
        (dict(pre_parts=1, pre_resid_rows=P), "pre_resid_rows without pre_resid"),
    ]
    for over, text in cases:
        _refused(pkg, who, call(**over), text, over)


def _struct(cls, optional, **vals):
    a = cls()
    for name, kind in a._fields_:
        if kind is C.c_void_p and name not in optional:
            setattr(a, name, 4096)
    for k, v in vals.items():
        setattr(a, k, v)
    return a


def test_head_out_refusals(pkg):
    lib, who = pkg.capi.load(), "ee_debug_head_out"
    lte_block = ("lte_in", "lte_gather", "lte_w", "lte_b", "lte_out")

    def call(lte=False, **over):
        vals = dict(in_rows=10, ld=128, H=128, Ko=2, max_docs=8, lte_rows=10, lte_ld=128, lte_split_inv=0.0)
        vals.update(over)
        return lib.ee_debug_head_out(C.byref(_struct(pkg.capi.DebugHeadOutArgs, () if lte else lte_block + ("gather",), **vals)), None)

    _refused(pkg, who, lib.ee_debug_head_out(None, None), "args must not be NULL", "args")
    null = "in, W, b, n_docs and out must not be NULL"
    counts = "bad counts (in_rows >= 1, 1 <= max_docs <= 2^20)"
    cases = [(dict([(k, None)]), null) for k in ("in_", "W", "b", "n_docs", "out")]
    cases += [
        (dict(W=None, H=3), null),                                              # the pointers before the sizes
        (dict(H=0), "hidden size 0 is not a multiple of 4 in [4, 1024]"), (dict(H=126), "hidden size 126 is not a multiple of 4 in [4, 1024]"),
        (dict(H=1028, ld=1028), "hidden size 1028 is not a multiple of 4 in [4, 1024]"),
        (dict(ld=124), "ld 124 is below the hidden size 128 or no multiple of 4"), (dict(ld=130), "ld 130 is below the hidden size 128 or no multiple of 4"),
        (dict(Ko=0), "Ko 0 is below 1"), (dict(Ko=-3), "Ko -3 is below 1"),
        (dict(in_rows=0), counts), (dict(max_docs=0), counts), (dict(max_docs=(1 << 20) + 1), counts),
        (dict(lte_w=4096), "the LTE block is given without lte_out"), (dict(lte_gather=4096), "the LTE block is given without lte_out"),
        (dict(lte=True, lte_in=None), "lte_out needs lte_in, lte_w and lte_b"), (dict(lte=True, lte_b=None), "lte_out needs lte_in, lte_w and lte_b"),
        (dict(lte=True, lte_ld=124), "lte_ld 124 is below the hidden size 128 or no multiple of 4"),
        (dict(lte=True, lte_ld=134), "lte_ld 134 is below the hidden size 128 or no multiple of 4"),
        (dict(lte=True, lte_rows=0), "lte_rows 0 is below 1"),
        (dict(lte=True, lte_split_inv=-1.0), "lte_split_inv must be 0 (f32 rows) or positive"),
        (dict(lte=True, lte_split_inv=float("nan")), "lte_split_inv must be 0 (f32 rows) or positive"),
        (dict(lte=True, lte_split_inv=0.0625, H=136, ld=136, lte_ld=136), "split rows need a hidden size that is a multiple of 16 (got 136)"),
    ]
    for over, text in cases:
        _refused(pkg, who, call(**over), text, over)


def test_exit_decide_refusals(pkg):
    lib, who = pkg.capi.load(), "ee_debug_exit_decide"
    optional = ("head_logits", "lte_score", "prev", "run", "out_logits", "out_conf", "out_all_logits", "out_all_crit", "out_head_logits", "out_head_crit",
                "meta_old", "meta_new", "row_src")

    def call(**over):
        vals = dict(mode=0, rule=0, criterion=0, K=4, Kh=2, thr=0.5, temp=1.0, patience=1, by_pointer=0, exit_index=0, is_final=0, no_exit=0, B=8)
        vals.update(over)
        return lib.ee_debug_exit_decide(C.byref(_struct(pkg.capi.DebugExitDecideArgs, optional, **vals)), None)

    _refused(pkg, who, lib.ee_debug_exit_decide(None, None), "args must not be NULL", "args")
    pair = ("launch_decide has no kernel for mode %d with rule %d (modes 0 threshold, 1 patience, 2 LTE; rules 0 plain, 1 streak, 2 either; patience "
            "takes the plain rule only)")
    crit = "criterion %d is none of MMEE_CRIT_MAX_CONFIDENCE, _ENTROPY, _MARGIN"
    cur = "pol_logits and the current stage (counts, doc_orig, doc_off, x_phys) must not be NULL"
    nxt = "the next stage (n_counts, n_doc_orig, n_doc_off, n_x_src, n_meta_src) and out_exit must not be NULL"
    state = "mode %d with rule %d keeps state per document: prev and run must be given"
    meta = "meta_old, meta_new and row_src are given together or not at all"
    cases = [(dict(mode=m, rule=r), pair % (m, r)) for m, r in ((-1, 0), (3, 0), (0, -1), (0, 3), (2, 3), (1, 1), (1, 2))]
    cases += [(dict(criterion=c), crit % c) for c in (-1, 2, 4)] + [(dict(mode=2, criterion=2), crit % 2)]
    cases += [
        (dict(mode=1, rule=1, K=0), pair % (1, 1)),                             # the pair is looked at first
        (dict(K=0), "K 0 or Kh 2 is below 1"), (dict(Kh=0), "K 4 or Kh 0 is below 1"),
        (dict(exit_index=-1), "exit_index -1 outside [0, 255]"), (dict(exit_index=256), "exit_index 256 outside [0, 255]"),
        (dict(B=0), "B 0 outside [1, 2^20]"), (dict(B=(1 << 20) + 1), "B 1048577 outside [1, 2^20]"),
        (dict(patience=-1), "patience -1 is negative"),
    ]
    cases += [(dict([(k, None)]), cur) for k in ("pol_logits", "counts", "doc_orig", "doc_off", "x_phys")]
    cases += [(dict([(k, None)]), nxt) for k in ("n_counts", "n_doc_orig", "n_doc_off", "n_x_src", "n_meta_src", "out_exit")]
    cases += [(dict(mode=m, rule=r, **given), state % (m, r)) for m, r in ((1, 0), (0, 1), (0, 2), (2, 1), (2, 2))
              for given in (dict(), dict(prev=4096), dict(run=4096))]
    cases += [(dict(given), meta) for given in (dict(meta_old=4096), dict(meta_new=4096), dict(row_src=4096), dict(meta_old=4096, meta_new=4096),
                                                dict(meta_new=4096, row_src=4096))]
    for over, text in cases:
        _refused(pkg, who, call(**over), text, over)


def test_rows_out_refusals(pkg):
    lib, who = pkg.capi.load(), "ee_debug_rows_out"

    def call(**over):
        vals = dict(which=0, x_rows=20, H=128, split_inv=0.0, max_docs=4, B=3, T=5, Pv=2, out_rows=30)
        vals.update(over)
        return lib.ee_debug_rows_out(C.byref(_struct(pkg.capi.DebugRowsOutArgs, (), **vals)), None)

    _refused(pkg, who, lib.ee_debug_rows_out(None, None), "args must not be NULL", "args")
    shape = "bad shape (B >= 1, T >= 0, Pv >= 0, T + Pv >= 1, B (T + Pv) <= 2^28), got B %d, T %d, Pv %d"
    cases = [
        (dict(which=2), "which 2 is neither 0 (gather_cls) nor 1 (rows_to_padded)"), (dict(which=-1), "which -1 is neither 0 (gather_cls) nor 1 (rows_to_padded)"),
        (dict(X=None), "X and out must not be NULL"), (dict(which=1, out=None), "X and out must not be NULL"),
        (dict(H=0), "hidden size 0 is not a multiple of 4 in [4, 4096]"), (dict(H=130), "hidden size 130 is not a multiple of 4 in [4, 4096]"),
        (dict(H=4100), "hidden size 4100 is not a multiple of 4 in [4, 4096]"),
        (dict(split_inv=-0.5), "split_inv must be 0 (f32 rows) or positive"), (dict(split_inv=float("nan")), "split_inv must be 0 (f32 rows) or positive"),
        (dict(split_inv=0.0625, H=136), "split rows need a hidden size that is a multiple of 16 (got 136)"),
        (dict(x_rows=0), "bad counts (x_rows >= 1, out_rows >= 0)"), (dict(which=1, out_rows=-1), "bad counts (x_rows >= 1, out_rows >= 0)"),
        (dict(x_phys=None), "gather_cls needs x_phys and n_docs"), (dict(n_docs=None), "gather_cls needs x_phys and n_docs"),
        (dict(max_docs=0), "max_docs 0 outside [1, 2^20]"), (dict(max_docs=(1 << 20) + 1), "max_docs 1048577 outside [1, 2^20]"),
        (dict(which=1, doc_off=None), "rows_to_padded needs doc_off"),
        (dict(which=1, B=0), shape % (0, 5, 2)), (dict(which=1, T=-1), shape % (3, -1, 2)), (dict(which=1, Pv=-1), shape % (3, 5, -1)),
        (dict(which=1, T=0, Pv=0), shape % (3, 0, 0)), (dict(which=1, B=1 << 20, T=1 << 9), shape % (1 << 20, 1 << 9, 2)),
        (dict(which=1, text_dst=None), "without text_dst (image-only) T must be 0, got 5"),
        (dict(which=1, ntext=None), "text_dst without ntext"),
    ]
    for over, text in cases:
        _refused(pkg, who, call(**over), text, over)


def test_patch_project_refusals(pkg):
    lib, who = pkg.capi.load(), "ee_debug_patch_project"
    err = C.c_int32(-1)

    def call(**over):
        vals = dict(B=2, C=3, R=64, P=16, H=256, form=0)
        vals.update(over)
        a = _struct(pkg.capi.DebugPatchProjectArgs, ("a_split_out",), **vals)
        a.err_flag_out = None if over.get("err_flag_out", 1) is None else C.pointer(err)
        return lib.ee_debug_patch_project(C.byref(a), None)

    _refused(pkg, who, lib.ee_debug_patch_project(None, None), "args must not be NULL", "args")
    null = "pixel_values, weight, bias, out and err_flag_out must not be NULL, B >= 1"
    geo = "unsupported patch geometry (R %% P == 0, P %% 4 == 0, R %% 4 == 0, C P P %% 32 == 0), got C %d, R %d, P %d"
    hidden = "hidden size %d is not a multiple of 128 in [128, 1024]"
    form = "form %d is none of 0 (f32, LDS-DMA kernel), 1 (f32, register-staged kernel), 2 (split)"
    split = "form 2 needs a shape gemm_split_supports takes (H %% 256 == 0, C P P %% 32 == 0), got H %d, C P P %d"
    cases = [(dict([(k, None)]), null) for k in ("pixel_values", "weight", "bias", "out", "err_flag_out")]
    cases += [
        (dict(B=0), null), (dict(B=-3), null), (dict(B=0, P=0), null),         # the pointers and B before the geometry
        (dict(R=72), geo % (3, 72, 16)),                                        # R % P
        (dict(C=2, R=36, P=6), geo % (2, 36, 6)), (dict(C=8, R=4, P=2), geo % (8, 4, 2)),      # P % 4, with C P P % 32 == 0
        (dict(C=1, R=48, P=12), geo % (1, 48, 12)), (dict(C=3, R=40, P=20), geo % (3, 40, 20)), (dict(C=1, R=32, P=4), geo % (1, 32, 4)),      # C P P % 32
        (dict(P=0), geo % (3, 64, 0)), (dict(C=0), geo % (0, 64, 16)), (dict(R=0), geo % (3, 0, 16)), (dict(P=-16), geo % (3, 64, -16)),
        (dict(R=72, H=100), geo % (3, 72, 16)),                                 # the geometry before the hidden size
        (dict(B=1 << 15, R=1024, P=4, C=2), "B (R / P)^2 = 2147483648 rows above 2^24, or B C R R above 2^30"),
        (dict(H=192), hidden % 192), (dict(H=0), hidden % 0), (dict(H=1152), hidden % 1152), (dict(H=192, form=7), hidden % 192),
        (dict(form=3), form % 3), (dict(form=-1), form % -1),
        (dict(form=2, H=128), split % (128, 768)), (dict(form=2, H=384), split % (384, 768)),
        (dict(a_split_out=4096), "a_split_out is written by form 2 only"), (dict(form=1, a_split_out=4096), "a_split_out is written by form 2 only"),
    ]
    for over, text in cases:
        _refused(pkg, who, call(**over), text, over)
    # every geometry class tests/pixel_ref.py lists passes the geometry rule: the checks BEHIND it are what refuses these calls, on the host
    from . import pixel_ref
    for (c, r, p), _ in pixel_ref.GEOMETRIES:
        _refused(pkg, who, call(C=c, R=r, P=p, H=192), hidden % 192, (c, r, p))
        _refused(pkg, who, call(C=c, R=r, P=p, form=3), form % 3, (c, r, p))
        _refused(pkg, who, call(C=c, R=r, P=p, H=128, form=2), split % (128, c * p * p), (c, r, p))


def test_gemm_routes_refusals(pkg):
    lib, who = pkg.capi.load(), "ee_debug_gemm_routes"
    optional = ("bias", "resid", "row_src", "resid_row_src", "col_scale")

    def call(**over):
        vals = dict(M=129, N=768, K=768, epi=0, out_split=0, a_scale=16.0, w_scale=256.0, out_scale=1.0, resid_scale=0.0, rows_A=300, rows_resid=0, route=0,
                    role_tag=0, probe=0, terms=3, k_splits=1, split_stride=0, scale_cols=0, scale=1.0, max_m=0, m_on_device=0, iters=1)
        vals.update(over)
        return lib.ee_debug_gemm_routes(C.byref(_struct(pkg.capi.DebugGemmRoutesArgs, optional, **vals)), None, None)

    _refused(pkg, who, lib.ee_debug_gemm_routes(None, None, None), "args must not be NULL", "args")
    bad = "bad argument (A, W, Cout not NULL, M, rows_A, iters >= 1, N % 256, K % 32, epi 0 .. 3, scales positive)"
    resid = "the residual epilogue needs resid, rows_resid >= 1 and resid_scale >= 0"
    parts = "k_splits %d is none of 1, 2, 4, 8"
    tail = "k_splits %d does not divide the %d k-stages of K = %d (the kernel would drop the last %d)"
    one = "k_splits %d needs the bias epilogue, an f32 output, three terms and no bias pointer (anything else writes one part)"
    cols = "scale_cols %d is not a multiple of 64 in [0, N = 768]"
    split = dict(k_splits=8, split_stride=(129 + 64) * 768)
    cases = [(dict([(k, None)]), bad) for k in ("A", "W", "Cout")]
    cases += [
        (dict(M=0), bad), (dict(rows_A=0), bad), (dict(iters=0), bad), (dict(N=128), bad), (dict(N=0), bad), (dict(K=48), bad), (dict(epi=4), bad),
        (dict(epi=-1), bad), (dict(a_scale=0.0), bad), (dict(w_scale=-1.0), bad), (dict(a_scale=float("nan")), bad), (dict(out_split=1, out_scale=0.0), bad),
        (dict(A=None, terms=2), bad),                                           # the pointers before everything else
        (dict(epi=2), resid), (dict(epi=2, resid=4096), resid), (dict(epi=2, resid=4096, rows_resid=300, resid_scale=-16.0), resid),
        (dict(terms=0), "terms 0 is neither 1 nor 3"), (dict(terms=2), "terms 2 is neither 1 nor 3"), (dict(terms=2, k_splits=3), "terms 2 is neither 1 nor 3"),
        (dict(k_splits=0), parts % 0), (dict(k_splits=3), parts % 3), (dict(k_splits=16), parts % 16), (dict(k_splits=-2), parts % -2),
        (dict(K=96, k_splits=2), tail % (2, 3, 96, 1)), (dict(K=96, k_splits=8), tail % (8, 3, 96, 3)), (dict(K=3232, k_splits=4), tail % (4, 101, 3232, 1)),
        (dict(K=128, k_splits=8), tail % (8, 4, 128, 4)),
        (dict(split, epi=1), one % 8), (dict(split, epi=3), one % 8), (dict(split, epi=2, resid=4096, rows_resid=300), one % 8),
        (dict(split, out_split=1), one % 8), (dict(split, terms=1), one % 8), (dict(split, bias=4096), one % 8), (dict(split, k_splits=2, bias=4096), one % 2),
        (dict(m_on_device=1, max_m=128), "M 129 is above max_m 128"), (dict(m_on_device=1), "M 129 is above max_m 0"),
        (dict(scale_cols=-64), cols % -64), (dict(scale_cols=100), cols % 100), (dict(scale_cols=832), cols % 832), (dict(scale_cols=255), cols % 255),
        (dict(route=3), "route 3 outside 0 / 1 / 2 or role_tag 0 none of 0, 2, 3"), (dict(role_tag=1), "route 0 outside 0 / 1 / 2 or role_tag 1 none of 0, 2, 3"),
        (dict(split, split_stride=129 * 768 - 1), "split_stride 99071 is below the 129 x 768 floats of a part"),
        (dict(split, m_on_device=1, max_m=300), "split_stride 148224 is below the 300 x 768 floats of a part"),
        (dict(rows_A=100), "M rows without a row map need M rows of A / of the residual"),
        (dict(epi=2, resid=4096, rows_resid=100), "M rows without a row map need M rows of A / of the residual"),
    ]
    for over, text in cases:
        _refused(pkg, who, call(**over), text, over)
    # the error word is an output like ms_out: asking for it changes no refusal
    err = C.c_int32(-1)
    for over, text in cases:
        a = _struct(pkg.capi.DebugGemmRoutesArgs, optional, **dict(dict(M=129, N=768, K=768, epi=0, out_split=0, a_scale=16.0, w_scale=256.0, out_scale=1.0,
                                                                        resid_scale=0.0, rows_A=300, rows_resid=0, route=0, role_tag=0, probe=0, terms=3,
                                                                        k_splits=1, split_stride=0, scale_cols=0, scale=1.0, max_m=0, m_on_device=0, iters=1),
                                                                   **over))
        a.err_flag_out = C.pointer(err)
        _refused(pkg, who, lib.ee_debug_gemm_routes(C.byref(a), None, None), text, ("err_flag_out", over))
    assert err.value == -1
    assert pkg.capi.DebugGemmRoutesArgs._fields_[-1][0] == "err_flag_out"          # appended: every field before it keeps its offset
    # what the hook lets through is what the rule of MMEE_FLAG_LOW_LATENCY produces: its S divides the k-stages (tests/test_host_gemm_routes.py)


def test_gemm_f32_refusals(pkg):
    lib, who = pkg.capi.load(), "ee_debug_gemm_f32"
    optional = ("bias", "resid", "row_src", "resid_row_src", "col_scale")

    def call(**over):
        vals = dict(M=129, N=256, K=64, epi=0, staging=0, use_queue=1, rows_A=300, rows_resid=0, scale_cols=0, scale=1.0, max_m=0, m_on_device=0,
                    wgs_per_cu=0)
        vals.update(over)
        return lib.ee_debug_gemm_f32(C.byref(_struct(pkg.capi.DebugGemmF32Args, optional, **vals)), None)

    _refused(pkg, who, lib.ee_debug_gemm_f32(None, None), "args must not be NULL", "args")
    null = "A, W and Cout must not be NULL"
    shape = "N %d is not a positive multiple of 128 or K %d not one of 32"
    epi = "epi %d outside 0 .. 3 (bias, GELU, residual, tanh; this hook takes no flag bits)"
    staging = "staging %d is neither 0 (LDS-DMA kernel) nor 1 (register-staged kernel)"
    other = "resid is read by the residual epilogue (epi 2) alone, got epi %d"
    cols = "scale_cols %d is not a multiple of 128 in [0, N = 256] (the kernel decides per 128-column tile side)"
    with_resid = dict(epi=2, resid=4096, rows_resid=300)
    cases = [(dict([(k, None)]), null) for k in ("A", "W", "Cout")]
    cases += [
        (dict(A=None, N=100), null),                                            # the pointers before everything else
        (dict(N=0), shape % (0, 64)), (dict(N=-128), shape % (-128, 64)), (dict(N=192), shape % (192, 64)), (dict(N=64), shape % (64, 64)),
        (dict(K=0), shape % (256, 0)), (dict(K=-32), shape % (256, -32)), (dict(K=48), shape % (256, 48)), (dict(K=16), shape % (256, 16)),
        (dict(N=192, M=-1), shape % (192, 64)),                                 # in the order of the entry point
        (dict(M=-1), "M -1 is negative"), (dict(M=-1, epi=7), "M -1 is negative"),
        (dict(epi=4), epi % 4), (dict(epi=-1), epi % -1), (dict(epi=256), epi % 256), (dict(epi=16 | 1), epi % 17),
        (dict(staging=2), staging % 2), (dict(staging=-1), staging % -1),
        (dict(epi=2), "the residual epilogue needs resid"),
        (dict(resid=4096), other % 0), (dict(epi=1, resid=4096), other % 1), (dict(epi=3, resid=4096, rows_resid=300), other % 3),
        (dict(scale_cols=-128), cols % -128), (dict(scale_cols=64), cols % 64), (dict(scale_cols=100), cols % 100), (dict(scale_cols=384), cols % 384),
        (dict(scale_cols=255), cols % 255),
        (dict(m_on_device=1), "max_m 0 is below 1"), (dict(m_on_device=1, max_m=-5), "max_m -5 is below 1"), (dict(M=0, m_on_device=1), "max_m 0 is below 1"),
        (dict(m_on_device=1, max_m=128), "M 129 is above max_m 128"), (dict(M=2, m_on_device=1, max_m=1), "M 2 is above max_m 1"),
        (dict(wgs_per_cu=-1), "wgs_per_cu -1 is negative (0: the default)"), (dict(with_resid, wgs_per_cu=-2), "wgs_per_cu -2 is negative (0: the default)"),
        (dict(rows_A=128), "M 129 rows without row_src need M rows of A, rows_A is 128"),
        (dict(with_resid, rows_resid=100), "M 129 rows without resid_row_src need M rows of the residual, rows_resid is 100"),
        (dict(with_resid, rows_A=100, rows_resid=100), "M 129 rows without row_src need M rows of A, rows_A is 100"),
    ]
    for over, text in cases:
        _refused(pkg, who, call(**over), text, over)


def test_split_rows_refusals(pkg):
    lib, who = pkg.capi.load(), "ee_debug_split_rows"
    err = C.c_int32(-1)

    def call(**over):
        a = dict(src=P, rows=3, K=256, scale=16.0, dst=P, err=C.byref(err))
        a.update(over)
        return lib.ee_debug_split_rows(*a.values(), None)

    null = "src, dst_words and err_flag_out must not be NULL"
    shape = "bad shape (rows >= 0, K a positive multiple of 16, rows K <= 2^30), got rows %d, K %d"
    scale = "scale must be positive and finite"
    cases = [
        (dict(src=None), null), (dict(dst=None), null), (dict(err=None), null), (dict(src=None, K=8), null),      # the pointers before the shape
        (dict(rows=-1), shape % (-1, 256)), (dict(K=0), shape % (3, 0)), (dict(K=8), shape % (3, 8)), (dict(K=24), shape % (3, 24)),
        (dict(K=-16), shape % (3, -16)), (dict(K=260), shape % (3, 260)), (dict(rows=1 << 23, K=256), shape % (1 << 23, 256)),
        (dict(K=24, scale=0.0), shape % (3, 24)),                               # the shape before the scale
        (dict(scale=0.0), scale), (dict(scale=-16.0), scale), (dict(scale=float("nan")), scale), (dict(scale=float("inf")), scale),
        (dict(scale=float("-inf")), scale),
    ]
    for over, text in cases:
        _refused(pkg, who, call(**over), text, over)
    assert err.value == -1


def test_split_weight_refusals(pkg):
    lib, who = pkg.capi.load(), "ee_debug_split_weight"
    inv = C.c_float(-1.0)

    def call(**over):
        a = dict(w=P, N=8, K=64, dst=P, inv=C.byref(inv))
        a.update(over)
        return lib.ee_debug_split_weight(*a.values(), None)

    null = "w, dst_words and inv_out must not be NULL"
    shape = "bad shape (N >= 1, K a positive multiple of 16, N K <= 2^30), got N %d, K %d"
    cases = [
        (dict(w=None), null), (dict(dst=None), null), (dict(inv=None), null), (dict(w=None, N=0), null),
        (dict(N=0), shape % (0, 64)), (dict(N=-2), shape % (-2, 64)), (dict(K=0), shape % (8, 0)), (dict(K=40), shape % (8, 40)),
        (dict(K=-64), shape % (8, -64)), (dict(N=1 << 20, K=2048), shape % (1 << 20, 2048)),
    ]
    for over, text in cases:
        _refused(pkg, who, call(**over), text, over)
    assert inv.value == -1.0
