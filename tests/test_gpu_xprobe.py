"""The X-space CLS probe alone (csrc/xprobe.hip: xprobe_u_kernel, xprobe_attn_kernel, xprobe_v_kernel) through ee_debug_xprobe, against the plain
float64 restatement of tests/xprobe_ref.py, for both instances (12 heads x 768, ring of 3; 16 x 1024, ring of 2), at every edge of the 16-row
tile loop, of the rank / u / value kernels' document groups and of the ticket loop.

Acceptance rule, per document (the project's, as test_gpu_attention.py): max |ctx - ref64| <= max(2 * yardstick, 1e-6), yardstick = the larger
error against float64 of the plain attention in torch float32 and of the X-space form in float32 with u, p, c through the planes
(xprobe_ref.yardstick); both sides decoded through the context planes.  tests/test_host_xprobe_ref.py shows that every listed mutation of the
kernel's steps moves the documents it concerns by at least 10 times that tolerance.  Every err, yardstick and err / tol is recorded with
report_measured before the assertion.

Bit-identity properties carry no tolerance: a document's context row does not depend on its neighbours, on its position in the stage, on the
number of workgroups (cus), on where its rows lie in xs, or on which form of the pair index the probe reads.  Every buffer the hook writes ends
in guard rows of a sentinel, and every context row that is not a document's doc_off row keeps the sentinel too.

Measured on an MI355X, worst err / tol (= err / (2 x yardstick)) over the documents of a case, 12 x 768 | 16 x 1024:
    tile edges 0.47 | 0.40      masked rows vs removed 0.45 | 0.40      staircases 0.32 | 0.40      plane scales of u 0.25 | 0.24
    tickets 0.38 | 0.35         stage indirection 0.33 | 0.35           document counts (24 launches, 700 documents of 1 .. 5 rows) 0.71 | 1.00
    intermediates at the tile edges: max |u - u64| / max |u64| 4.7e-8 | 4.8e-8, max |c - c64| / max |c64| 1.1e-6 | 1.8e-6
The documents of a few rows at |x| ~ 4 are the hard ones: their context is as large as a V row (|ctx| ~ 10, a float32 ulp of 1e-6) and a float32
error of a score of 30 goes into it undamped.  The worst, count[16 x 1024, n = 17] document 11 (3 rows), sits AT the bound: err 1.335e-5 =
2 x yardstick 6.676e-6 (14 and 7 steps of the context planes).  Before the probe's kernels summed u in float64 and split their accumulators
(csrc/xprobe.hip) these cases missed the rule: a one-row document at the tile edges by 1.14 x tol (12 x 768), and documents of 2 .. 4 rows in
seven of the 24 count launches by up to 1.82 x tol (smallest: n = 9 at 16 x 1024, n = 15 at 12 x 768, two rows)."""
import ctypes as C
import functools

import numpy as np
import pytest

from . import attn_ref as R
from . import xprobe_ref as X
from .conftest import report_measured
from .hook_util import ERR_SPLIT_OVERFLOW, SENTINEL, _stream, _torch

pytestmark = pytest.mark.gpu

HEADS = [12, 16]
GUARD = 8                                               # rows past the last one in every output buffer; they must keep SENTINEL's bits
hid = lambda h: f"{h}x{64 * h}"


def _dev(a, dtype):
    """A device copy, never empty: the hook refuses NULL pointers also where a count is 0."""
    torch = _torch()
    a = np.ascontiguousarray(a)
    if a.size == 0:
        a = np.zeros((1,) + a.shape[1:], a.dtype)
    return torch.from_numpy(a).to(device="cuda", dtype=dtype)


class Out:
    pass


def _launch(pkg, c, cus=0, index_form=0, expect_err=0, refused=False, **over):
    """One ee_debug_xprobe call on case c.  Returns ctx as the kernels wrote it (int32 words [ctx_rows, H], on the device) and the intermediates;
    checks the error word, the guard rows and that only the doc_off rows of ctx were written.  refused: the call must fail, and write nothing."""
    torch = _torch()
    o, H, nh, n = c.orig, c.H, c.heads, c.n_docs
    i32, f32 = torch.int32, torch.float32
    keep = dict(orig_doc_off=_dev(o.doc_off, i32), pos=_dev(o.pos, i32), x0=_dev(o.x0, i32), y1=_dev(o.y1, i32), masked=_dev(o.masked, i32),
                doc_off=_dev(over.pop("doc_off", c.doc_off), i32), doc_orig=_dev(over.pop("doc_orig", c.doc_orig), i32),
                x_phys=_dev(over.pop("x_phys", c.x_phys), i32), xs=_dev(X.encode_planes(c.xs, X.SCALE_X), i32), qc=_dev(c.qc, f32),
                wk=_dev(c.wk, f32), bk=_dev(c.bk, f32), bv=_dev(over.pop("bv", c.bv), f32), wv=_dev(c.wv, f32), w1=_dev(o.w1, f32), wx=_dev(o.wx, f32),
                wy=_dev(o.wy, f32))
    full = lambda rows, cols: torch.full((rows + GUARD, cols), SENTINEL, dtype=i32, device="cuda")
    outs = dict(ctx=full(c.ctx_rows, H), u_out=full(n * nh, H), s0_out=full(n * nh, 2), cvec_out=full(n * nh, H), order_out=full(n, 1))
    a = pkg.capi.DebugXProbeArgs()
    for k, t in list(keep.items()) + list(outs.items()):
        setattr(a, k, t.data_ptr())
    vals = dict(n_orig=o.n_docs, n_docs=n, max_docs=c.max_docs, x_rows=len(c.xs), ctx_rows=c.ctx_rows, H=H, heads=nh, bins1=o.w1.shape[1], bins2=o.wx.shape[1],
                max_rel_pos=R.MAX_REL_POS, max_rel_2d_pos=R.MAX_REL_2D_POS, max_pos=o.max_pos, max_coord=R.MAX_COORD, index_form=index_form, cus=cus)
    vals.update(over)
    for k, v in vals.items():
        setattr(a, k, v)
    err = C.c_int32(-1)
    rc = pkg.capi.load().ee_debug_xprobe(C.byref(a), C.byref(err), _stream())
    torch.cuda.synchronize()
    if refused:
        assert rc != 0, "the hook accepted what it must refuse"
        for k, t in outs.items():
            assert torch.equal(t, torch.full_like(t, SENTINEL)), f"a refused call wrote to {k}"
        return pkg.capi.last_error()
    pkg.capi.check(rc, None, "ee_debug_xprobe")
    assert err.value == expect_err, f"err_flag {err.value}"
    r = Out()
    sizes = dict(ctx=c.ctx_rows, u_out=n * nh, s0_out=n * nh, cvec_out=n * nh, order_out=n)
    for k, t in outs.items():
        assert torch.equal(t[sizes[k]:], torch.full_like(t[sizes[k]:], SENTINEL)), f"a write past the end of {k}"
    r.ctx = outs["ctx"][:c.ctx_rows]
    other = torch.ones(c.ctx_rows, dtype=torch.bool, device="cuda")
    if n:
        other[_dev(c.doc_off[:-1].astype(np.int64), torch.int64)] = False
    assert torch.equal(r.ctx[other], torch.full_like(r.ctx[other], SENTINEL)), "a context row that is no document's doc_off row was written"
    r.rows = r.ctx[_dev(c.doc_off[:-1].astype(np.int64), torch.int64)] if n else r.ctx[:0]            # [n_docs, H] words
    r.u = outs["u_out"][:n * nh].view(f32).reshape(n, nh, H)
    r.s0 = outs["s0_out"][:n * nh].view(f32).reshape(n, nh, 2)
    r.cvec = outs["cvec_out"][:n * nh].view(f32).reshape(n, nh, H)
    r.order = outs["order_out"][:n, 0]
    return r


def _values(words):
    return X.decode_planes(words.cpu().numpy(), X.SCALE_CTX)


@functools.lru_cache(maxsize=None)
def _shared(kind, heads, *args):
    """A case of xprobe_ref, its float64 reference and the yardstick per document: computed once, shared by every test, never written to."""
    c = getattr(X, kind + "_case")(heads, *args)
    ref = X.reference(c)
    return c, ref, X.yardstick(c, ref)


def _check(tag, c, got, ref, yard):
    """The acceptance rule on every document; every err, yardstick and err / tol is recorded before the assertion."""
    bad = []
    for d, L in enumerate(c.lengths):
        err = float(np.abs(got[d] - ref[d]).max())
        tol = float(R.tolerance(yard[d]))
        report_measured(f"xprobe[{tag},d={d},L={L}]", f"max|err| (yardstick {yard[d]:.3e}, err / yardstick {err / max(yard[d], 1e-30):.2f}, err / tol {err / tol:.2f})", err)
        if not err <= tol:
            bad.append((d, int(L), err, float(yard[d])))
    assert not np.isnan(got).any()
    assert not bad, (tag, bad)


def _check_order(c, r):
    assert np.array_equal(r.order.cpu().numpy(), X.order_ref(c.lengths)), "order is not (length descending, index ascending)"


def _intermediates(tag, c, r):
    """u of every document against its float64 value, asserted: the kernel sums the 64 products of an element in float64 and rounds ONCE to
    float32, so |u - u64| <= 2^-24 |u64| (that rounding) + 128 x 2^-53 x sum |q| |w| (the float64 sum, generously) + 2^-126 (a flushed subnormal); a
    float32 fma chain, which put 2e-5 into the contexts of short documents, misses this by a factor of ten and more.  c against its float64
    value is RECORDED only, not asserted (it says which step is off when the rule fails): its bound is the acceptance rule on the context."""
    nh, H = c.heads, c.H
    wk = c.wk.astype(np.float64).reshape(nh, 64, H)
    u, cv = r.u.cpu().numpy().astype(np.float64), r.cvec.cpu().numpy().astype(np.float64)
    worst_u = worst_c = 0.0
    for d in range(c.n_docs):
        q = c.qc[d].astype(np.float64).reshape(nh, 64)
        u64 = np.einsum("hd,hdc->hc", q, wk)
        bound = 2.0 ** -24 * np.abs(u64) + 128 * 2.0 ** -53 * np.einsum("hd,hdc->hc", np.abs(q), np.abs(wk)) + 2.0 ** -126
        assert (np.abs(u[d] - u64) <= bound).all(), f"u of document {d}"
        worst_u = max(worst_u, float((np.abs(u[d] - u64) / (np.abs(u64).max() + 1e-300)).max()))
        p = X.reference_doc(c, d)[2]
        c64 = p @ c.X(d)
        worst_c = max(worst_c, float((np.abs(cv[d] - c64).max() / np.abs(c64).max())))
    report_measured(f"xprobe[{tag}]", "max |u - u64| / max |u64|", worst_u)
    report_measured(f"xprobe[{tag}]", "max |c - c64| / max |c64|", worst_c)


# ---------------------------------------------------------------------------------------------------------------------------------------
# accuracy
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("heads", HEADS, ids=hid)
def test_probe_against_float64_at_every_tile_edge(pkg, heads):
    """Lengths 1 ... 709 in one launch: one row, partial and full last tiles, 1 to 45 tiles through both rings, holes from 33 rows on, a document
    whose whole tile 1 is masked, one with masked pad rows behind its text."""
    c, ref, yard = _shared("edge", heads)
    r = _launch(pkg, c)
    _check_order(c, r)
    _intermediates(f"edge,{hid(heads)}", c, r)
    _check(f"edge,{hid(heads)}", c, _values(r.rows), ref, yard)


@pytest.mark.parametrize("heads", HEADS, ids=hid)
def test_masked_rows_do_not_leak(pkg, heads):
    """The masked rows of the edge batch hold values at the top of the plane range: the result matches the same batch with those rows removed, to
    the acceptance rule (against the removed batch's float64 reference and yardstick), and so does the removed batch itself."""
    c = _shared("edge", heads)[0]
    c2 = X.without_masked_rows(c)
    ref2 = X.reference(c2)
    yard2 = X.yardstick(c2, ref2)
    _check(f"masked rows vs removed,{hid(heads)}", c, _values(_launch(pkg, c).rows), ref2, yard2)
    _check(f"masked rows removed,{hid(heads)}", c2, _values(_launch(pkg, c2).rows), ref2, yard2)


@pytest.mark.parametrize("heads", HEADS, ids=hid)
def test_lazy_maximum_staircases(pkg, heads):
    """Tile maxima that rise by 4.9 and 5.1 log2 units (cumulative 0, 4.9, 9.8: no move, then a move), by several hundred (the old accumulator
    underflows to 0), that fall, and that go up and down; odd heads run the sequences backwards, so the heads of a wave move at different tiles."""
    c, ref, yard = _shared("staircase", heads)
    _check(f"staircase,{hid(heads)}", c, _values(_launch(pkg, c).rows), ref, yard)


@pytest.mark.parametrize("heads", HEADS, ids=hid)
def test_degenerate_plane_scales_of_u(pkg, heads):
    """q = 0 (u = 0, plane scale 1: the context is the bias-weighted mean) and a large q (scores in the hundreds) next to an ordinary document."""
    c, ref, yard = _shared("scale", heads)
    r = _launch(pkg, c)
    assert (r.s0[0, :, 1] == 1.0).all() and (r.s0[0, :, 0] == 0.0).all() and not r.u[0].any()
    _check(f"scale,{hid(heads)}", c, _values(r.rows), ref, yard)


@pytest.mark.parametrize("n_docs,equal", [(1, False), (7, False), (8, False), (9, False), (15, False), (16, False), (17, False), (63, False), (64, False),
                                          (65, False), (33, True), (65, True)])
@pytest.mark.parametrize("heads", HEADS, ids=hid)
def test_document_counts(pkg, heads, n_docs, equal):
    """Short documents (1 .. 5 rows) at every edge of the u kernel's groups of 8 and of the value kernel's 16 per wave / 64 per block; runs of
    equal lengths for the stride and the tie rule of the rank loop.  order is exact."""
    c, ref, yard = _shared("count", heads, n_docs, equal)
    r = _launch(pkg, c)
    _check_order(c, r)
    _check(f"count,{hid(heads)},n={n_docs}{',equal' if equal else ''}", c, _values(r.rows), ref, yard)


# ---------------------------------------------------------------------------------------------------------------------------------------
# several documents per workgroup; the stage's indirections; bit identity
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("heads", HEADS, ids=hid)
def test_one_workgroup_processes_several_documents(pkg, heads):
    """Nine documents alternating long and short with one and two workgroups: a short document follows a long one on the same LDS ring, bias
    tables and bucket bytes.  The same bits as at the device's CU count, which meet the rule."""
    torch = _torch()
    c, ref, yard = _shared("ticket", heads)
    full = _launch(pkg, c)
    _check_order(c, full)
    _check(f"ticket,{hid(heads)}", c, _values(full.rows), ref, yard)
    for cus in (1, 2):
        r = _launch(pkg, c, cus=cus)
        assert torch.equal(r.rows, full.rows), f"cus = {cus} and the device's count differ"
        assert torch.equal(r.order, full.order)
    assert torch.equal(_launch(pkg, c).rows, full.rows), "two launches differ"


@pytest.mark.parametrize("heads", HEADS, ids=hid)
def test_stage_indirection(pkg, heads):
    """A stage that is a shuffled subset of 7 of 12 original documents, its rows scattered in xs with gaps and out of order: the pair-index slab is
    doc_orig[d]'s, the rows are read at x_phys[d], the context row is written at doc_off[d] and nowhere else; every cus value gives the same
    bits.  (The second form of the pair index: test_both_forms_of_the_pair_index_give_the_same_bits.)"""
    torch = _torch()
    c, ref, yard = _shared("stage", heads)
    assert not np.array_equal(c.doc_orig, np.arange(c.n_docs)) and (np.diff(c.x_phys) < 0).any() and c.max_docs > c.n_docs
    full = _launch(pkg, c)
    _check_order(c, full)
    _check(f"stage,{hid(heads)}", c, _values(full.rows), ref, yard)
    for cus in (1, 2):
        assert torch.equal(_launch(pkg, c, cus=cus).rows, full.rows), f"cus = {cus} and the device's count differ"
    msg = _launch(pkg, c, index_form=1, refused=True)               # the release library holds no 16-bit pair index: refused, nothing launched
    assert "index_form 1 needs the diagnostic library" in msg, msg


def _form1_child():
    """Runs in a child process whose MMEE_LIB is the diagnostic library (test_both_forms_of_the_pair_index_give_the_same_bits)."""
    import importlib
    torch = _torch()
    pkg = importlib.import_module("multi-modal-early-exit_amd")
    assert pkg.capi.lib_path().endswith("libmmee_hip_diag.so"), pkg.capi.lib_path()
    for heads in HEADS:
        c = X.stage_case(heads)
        ref = X.reference(c)
        full = _launch(pkg, c)
        _check(f"stage (diagnostic library),{hid(heads)}", c, _values(full.rows), ref, X.yardstick(c, ref))
        for cus in (0, 1):
            r1 = _launch(pkg, c, index_form=1, cus=cus)
            assert torch.equal(r1.rows, full.rows), f"the two forms of the pair index differ ({heads} heads, cus = {cus})"
            assert torch.equal(r1.order, full.order)
        wide = X.stage_case(heads)                               # 72 bins of the 1-D table: the probe takes them (its LDS layout still fits), the 16-bit index holds 64
        wide.orig.w1 = np.concatenate([wide.orig.w1, wide.orig.w1, wide.orig.w1[:, :8]], axis=1)
        msg = _launch(pkg, wide, index_form=1, refused=True)
        assert "attention_idx16_fits refuses 72" in msg, msg
        _launch(pkg, wide)                                       # ... and the 32-bit form runs them
    print("FORM1_OK")


def test_both_forms_of_the_pair_index_give_the_same_bits(pkg):
    """index_form 1 (the query-block-0 output of launch_pair_index16, slab stride nb x 1024) exists in the DIAGNOSTIC library only, as the forward's
    16-bit index does (test_gpu_round6.py): a child process on that library runs the stage case with both forms at cus = 0 and cus = 1 and
    compares the context words bit for bit, and checks the attention_idx16_fits refusal."""
    import os
    import subprocess
    import sys
    from .conftest import ROOT
    diag = os.path.join(ROOT, "multi-modal-early-exit_amd", "libmmee_hip_diag.so")
    # build() makes only the release library: a fresh checkout builds the diagnostic one here (make is a no-op when it is up to date)
    subprocess.run(["make", "-C", os.path.join(ROOT, "multi-modal-early-exit_amd", "csrc"), "diag", "-j8"], check=True, stdout=subprocess.DEVNULL)
    r = subprocess.run([sys.executable, "-c", "from tests import test_gpu_xprobe as T; T._form1_child()"], cwd=ROOT, env=dict(os.environ, MMEE_LIB=diag),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "FORM1_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


@pytest.mark.parametrize("heads", HEADS, ids=hid)
def test_a_documents_context_depends_on_nothing_but_the_document(pkg, heads):
    """The same documents in another stage order, at other places of xs (x_phys), and each alone in a stage of one: the same bits per document."""
    torch = _torch()
    c = _shared("stage", heads)[0]
    full = _launch(pkg, c)
    perm = [4, 0, 6, 2, 5, 1, 3]
    docs = [X.STAGE_DOCS[i] for i in perm]
    lens = [X.STAGE_ORIG_LENGTHS[o] for o in docs]
    x_phys = np.concatenate([[3], 3 + np.cumsum(np.array(lens[:-1]) + 5)])                  # packed from row 3 on, five rows between documents
    assert x_phys[-1] + lens[-1] <= X.STAGE_X_ROWS
    c2 = X.stage_case(heads, tuple(docs), tuple(int(x) for x in x_phys))
    r2 = _launch(pkg, c2, cus=2)
    for i, j in enumerate(perm):
        assert torch.equal(r2.rows[i], full.rows[j]), f"document {X.STAGE_DOCS[j]} changed with its position / x_phys"
    for j in (0, 3, 6):
        c1 = X.stage_case(heads, (X.STAGE_DOCS[j],), (X.STAGE_X_PHYS[j],))
        assert torch.equal(_launch(pkg, c1).rows[0], full.rows[j]), f"document {X.STAGE_DOCS[j]} alone differs"


# ---------------------------------------------------------------------------------------------------------------------------------------
# the empty stage, the overflow flag, refusals
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("heads", HEADS, ids=hid)
def test_empty_stage(pkg, heads):
    """n_docs = 0 with max_docs = 8: the launches return (the ticket counter of a dirty workspace is reset), ctx is untouched, err_flag is 0."""
    c = X.stage_case(heads, (), ())
    c.max_docs = 8
    r = _launch(pkg, c)                     # _launch asserts that no row of ctx was written and that err_flag is 0
    assert r.rows.shape[0] == 0


@pytest.mark.parametrize("heads", HEADS, ids=hid)
def test_overflow_raises_the_flag_and_changes_nothing_else(pkg, heads):
    """b_v[5] = 1000: 1000 x 64 > kSplitClamp raises kErrSplitOverflow; every other column keeps its bits."""
    torch = _torch()
    c = _shared("scale", heads)[0]
    base = _launch(pkg, c).rows
    bv = c.bv.copy()
    bv[5] = 1000.0
    got = _launch(pkg, c, bv=bv, expect_err=ERR_SPLIT_OVERFLOW).rows
    h_base, h_got = base.view(torch.float16).clone(), got.view(torch.float16).clone()        # column 5: f16 5 (hi) and 21 (lo) of the first group
    assert not torch.equal(h_base[:, 5], h_got[:, 5])
    for h in (h_base, h_got):
        h[:, 5] = 0
        h[:, 21] = 0
    assert torch.equal(h_base.view(torch.int32), h_got.view(torch.int32))


def test_refusals(pkg):
    """What xprobe_supports refuses, and what would leave the caller's buffers: an error, and nothing launched (no output byte changes)."""
    msg = _launch(pkg, X.count_case(8, 1), refused=True)
    assert "xprobe_supports refuses 8 heads x 512" in msg, msg
    c12 = X.count_case(12, 3)
    msg = _launch(pkg, c12, refused=True, H=1024)
    assert "xprobe_supports refuses 12 heads x 1024" in msg, msg
    msg = _launch(pkg, c12, refused=True, bins1=256)
    assert "xprobe_supports refuses" in msg and "256" in msg, msg
    big = X.identity_case(R.make_batch((833,), 12, seed=3, holes=False), seed=4)              # npad = 848: the layout needs 163,888 bytes
    msg = _launch(pkg, big, refused=True)
    assert "xprobe_supports refuses" in msg and "max_len 833" in msg, msg
    st = X.stage_case(12)
    off = st.doc_off.copy()
    off[1] += 1                                                                              # one row moves from document 1 to document 0
    msg = _launch(pkg, st, refused=True, doc_off=off)
    assert "its original" in msg, msg
    xp = st.x_phys.copy()
    xp[2] = X.STAGE_X_ROWS - 40                                                              # document 2 has 48 rows
    msg = _launch(pkg, st, refused=True, x_phys=xp)
    assert "leave the 760 rows of xs" in msg, msg
    do = st.doc_orig.copy()
    do[0] = 12
    msg = _launch(pkg, st, refused=True, doc_orig=do)
    assert "outside the 12 original documents" in msg, msg
