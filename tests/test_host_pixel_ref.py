"""The restatement of the pixel path (tests/pixel_ref.py), checked without a GPU: its resize equals Pillow (the fixture always, Pillow itself
where it is installed), its models of the kernels' arithmetic equal its references, and the inputs of tests/test_gpu_pixel.py can SEE a
subtly wrong kernel -- every fault below changes at least one byte of a resize or collation output, or moves a row of the projection by
more than 10 times the tolerance that row is held to.  That tolerance is max(2 err32, 1e-6); here err32 is torch's float32 product on the
CPU, on the GPU it is the larger of torch's GEMM and the k-sequential float32 loop; the GPU tolerance of a case's worst row measured at most
8.5 times the smallest CPU tolerance of a row of that case, so the projection faults are asked to move a row by 1000 times the CPU tolerance."""
import ctypes as C

import numpy as np
import pytest

from . import pixel_ref as X
from .conftest import load_golden

MARGIN = 1000.0


# ---- resize ----------------------------------------------------------------------------------------------------------------------------
def test_the_resize_restatement_equals_the_pillow_fixture(pkg):
    g = load_golden("preprocess_edges")
    assert [tuple(int(v) for v in c) for c in g["cases"]] == [(R,) + s for R, s in X.GOLDEN_CASES]
    for i, (R, s) in enumerate(X.GOLDEN_CASES):
        u8, px = X.resize_ref(X.make_page(pkg.synth, R, s), R)
        assert np.array_equal(u8, g[f"res{i}"]), (R, s)
        assert px.dtype == np.float32 and px.shape == (3, R, R) and np.array_equal(px[1, 0], X.rescale_normalize_lut()[u8[0, :, 1]])


def test_the_resize_restatement_equals_pillow_at_every_shape(pkg):
    Image = pytest.importorskip("PIL.Image")
    for R, s in X.RESIZE_CASES + [(X.MIXED_CALL[0], t) for t in X.MIXED_CALL[1]]:
        page = X.make_page(pkg.synth, R, s)
        want = np.asarray(Image.fromarray(page).convert("RGB").resize((R, R), resample=Image.BILINEAR))
        assert np.array_equal(X.resize_ref(page, R)[0], want), (R, s)


def test_the_resize_shapes_are_the_edges_they_are_listed_for():
    shapes = {R: [s for r, s in X.RESIZE_CASES if r == R] for R in (224, 32, 1, 3, 7)}
    hs = [h for h, _, _ in shapes[224]]
    sweeps = lambda h: -(-(h * 224) // (1024 * 256))                 # resize_first_pass_kernel: 1024 blocks of 256 threads per sweep
    assert sweeps(1170) == 1 and sweeps(1171) == 2 and sweeps(2400) == 3 and 1171 in hs and 2400 in hs
    assert max(max(h, w) for h, w, _ in shapes[224]) == X.MAX_RATIO * 224 and (992, 992, 1) in shapes[32] and 992 == X.MAX_RATIO * 32
    assert {1, 2} <= set(hs) and {1, 3} <= {w for _, w, _ in shapes[224]}
    assert {c for _, _, c in shapes[224]} == {1, 3}
    assert [s for s in shapes[224] if X.vertical_first(s[0], s[1], 224)] == [(500, 1, 3), (6944, 8, 1)]      # Image.resize's other pass order
    hm = [h for h, _, _ in X.MIXED_CALL[1]]
    assert hm.index(max(hm)) != 0 and hm[-1] < hm[-2] and {c for _, _, c in X.MIXED_CALL[1]} == {1, 3}


def _pages(pkg, R, shapes):
    return [X.make_page(pkg.synth, R, s) for s in shapes]


def test_the_resize_model_equals_the_reference(pkg):
    for R, s in X.GOLDEN_CASES + [(224, (447, 449, 3)), (224, (225, 223, 1)), (224, (6944, 8, 1))]:
        page = X.make_page(pkg.synth, R, s)
        assert np.array_equal(X.resize_model([page], R)[0], X.resize_ref(page, R)[0]), (R, s)
    R, shapes = X.MIXED_CALL
    pages = [p for p, s in zip(_pages(pkg, R, shapes), shapes) if s[0] <= 300]              # the mixed call's short pages: a plane stride above every height but one
    got = X.resize_model(pages, R, align=1, lead=3)
    for i, p in enumerate(pages):
        assert np.array_equal(got[i], X.resize_ref(p, R)[0]), i


# fault -> the cases that must see it: (R, pages of one call)
RESIZE_SEES = {
    "no_rounding": [(224, [(223, 225, 3)]), (32, [(33, 65, 3)]), (7, [(17, 5, 3)])],
    "plane_stride_h": [(224, [(300, 224, 1), (2, 3, 3)])],                                  # as in the mixed call: a short page behind a tall one
    "xmax_unclipped": [(224, [(223, 225, 3)]), (32, [(33, 65, 3)]), (7, [(17, 5, 3)]), (224, [(2, 3, 3)])],
    "unnormalised": [(224, [(447, 449, 3)]), (32, [(33, 65, 3)]), (3, [(93, 93, 1)]), (1, [(31, 31, 3)])],
    "grey_channel0_only": [(224, [(225, 223, 1)]), (3, [(93, 93, 1)]), (224, [(1, 1, 1)])],
    "horizontal_always": [(224, [(6944, 8, 1)])],                                           # Image.resize runs the vertical pass first for this page
}


@pytest.mark.parametrize("fault", X.RESIZE_FAULTS)
def test_the_resize_cases_see_a_subtle_fault(pkg, fault):
    for R, shapes in RESIZE_SEES[fault]:
        assert all((R, s) in X.RESIZE_CASES or (R == X.MIXED_CALL[0] and s in X.MIXED_CALL[1]) for s in shapes)
        pages = _pages(pkg, R, shapes)
        differing = int((X.resize_model(pages, R, fault) != X.resize_model(pages, R)).sum())
        print(f"{fault}: R {R} {shapes}: {differing} bytes differ")
        assert differing >= 1, (fault, R, shapes)


def test_preprocess_refuses_a_page_taller_than_the_tap_tables(pkg):
    lib, p = pkg.capi.load(), C.c_void_p(4096)
    assert lib.ee_preprocess_images(p, p, 1, 32, 31 * 32 + 1, p, 1 << 30, p, None, None) != 0
    assert pkg.capi.last_error() == "ee_preprocess_images: max_h 993 is above 31 R = 992 (the tap tables hold 64 taps per output pixel)"
    assert lib.ee_preprocess_workspace_bytes(1, 32, 992) > 992 * 32 * 3


# ---- collation -------------------------------------------------------------------------------------------------------------------------
def _collate_cases():
    for T in X.COLLATE_T:
        for B in X.COLLATE_B:
            for i, lengths in enumerate(X.collate_lengths(B, T)):
                for pad in X.COLLATE_PAD:
                    yield T, B, lengths, pad, 1000 * T + 10 * B + i


def test_the_collation_cases_are_the_edges_they_are_listed_for():
    for T in X.COLLATE_T:
        assert sorted(set(sum(X.collate_lengths(1, T), []))) == sorted({0, 1, T - 1, T, T + 1, 5 * T})
        many = X.collate_lengths(7, T)[0]
        assert many[0] == 0 and many[-1] == 0 and {1, T - 1, T, T + 1, 5 * T} <= set(many)
    ids, boxes, off = X.collate_inputs([5, 0, 600], 3)
    assert (ids >= X.BIG).any() and (boxes >= X.BIG).any() and (ids < 0).any() and off.tolist() == [0, 5, 5, 605]
    got = X.collate_ref(ids, boxes, off, 8, -7)
    assert got[0][0].tolist() == ids[:5].tolist() + [-7] * 3 and got[1].sum(1).tolist() == [5, 0, 8] and (got[2][1] == 0).all()
    assert np.array_equal(got[2][2], boxes[5:13]) and np.array_equal(got[0][2], ids[5:13])


@pytest.mark.parametrize("fault", X.COLLATE_FAULTS)
def test_the_collation_cases_see_a_subtle_fault(fault):
    seen = 0
    for T, B, lengths, pad, seed in _collate_cases():
        ids, boxes, off = X.collate_inputs(lengths, seed)
        ref, bad = X.collate_ref(ids, boxes, off, T, pad), X.collate_model(ids, boxes, off, T, pad, fault)
        seen += any(not np.array_equal(a, b) for a, b in zip(ref, bad))
    print(f"{fault}: seen by {seen} cases")
    assert seen >= 1


# ---- patch projection ------------------------------------------------------------------------------------------------------------------
def test_the_geometries_are_the_classes_ee_create_accepts():
    for (C_, R, P), _ in X.GEOMETRIES:
        assert R % P == 0 and P % 4 == 0 and R % 4 == 0 and (C_ * P * P) % 32 == 0
    geos = [g for g, _ in X.GEOMETRIES]
    assert {P for _, _, P in geos if 32 % P} == {12, 20} and {P for _, _, P in geos if (P * P) % 32} == {4, 12, 20}
    rows = [B * (R // P) ** 2 for (_, R, P), bs in X.GEOMETRIES for B in bs]
    assert 196 in rows and 588 in rows and {127, 128, 129} <= set(rows) and any(m % X.TILE for m in rows)


@pytest.mark.parametrize("geo,B", X.project_cases(), ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_the_im2col_model_equals_the_reference(geo, B):
    pix, W, b = X.project_operands(geo, B, 128, "lut")
    A = X.im2col(pix, geo[2])
    assert np.array_equal(X.im2col_model(pix, geo[2]), A)
    assert np.array_equal(X.decode_words(X.split_words(pix, geo[2])), X.split_values(pix, geo[2]))
    err32 = X.per_row_max(X.split_values(pix, geo[2]) - A.astype(np.float64))
    assert err32.max() <= 2.0 ** -21                                       # 22 bits of a value below 2
    assert np.abs(pix).max() * X.SPLIT_SCALE < X.SPLIT_LIMIT < 5000.0 * X.SPLIT_SCALE


# fault -> the geometries that must see it (the others may: at P = 16 a slab never leaves its channel and kx never changes)
PROJECT_SEES = {
    "kx_first_slab": [(2, 48, 12), (2, 24, 12), (2, 40, 20)],
    "c_from_k0": [(6, 32, 4), (2, 48, 12), (2, 24, 12), (2, 40, 20)],
    "channel_stride_dropped": [g for g, _ in X.GEOMETRIES if g[0] > 1],
    "image_of_tile_first_row": [(3, 224, 16), (3, 16, 16), (6, 32, 4), (2, 24, 12)],
}


@pytest.mark.parametrize("draw", ["lut", "general"])
@pytest.mark.parametrize("fault", X.PROJECT_FAULTS)
def test_the_projection_cases_see_a_subtle_fault(fault, draw):
    for geo in PROJECT_SEES[fault]:
        B = max(dict(X.GEOMETRIES)[geo])
        pix, W, b = X.project_operands(geo, B, 128, draw)
        ref = X.project_ref(pix, W, b, geo[2])
        tol = X.tolerance(X.per_row_max(X.project_f32_torch(pix, W, b, geo[2]).astype(np.float64) - ref))
        bad = X.im2col_model(pix, geo[2], fault).astype(np.float64) @ W.astype(np.float64).T + b
        ratio = float((X.per_row_max(bad - ref) / tol).max())
        print(f"{fault}, {draw}, {geo} B {B}: a row moves by {ratio:.1f} x its tolerance")
        assert ratio >= MARGIN, (fault, geo, ratio)
        split = X.split_round(X.im2col_model(pix, geo[2], fault), X.SPLIT_SCALE)      # the same fault in patch_split_kernel: the rows differ
        assert not np.array_equal(split, X.split_values(pix, geo[2]))


def test_the_guard_rows_see_an_unmasked_store():
    ms = [B * (R // P) ** 2 for (_, R, P), bs in X.GEOMETRIES for B in bs]
    assert X.GUARD >= 1 and all(X.rows_written(m) == m for m in ms)
    assert sum(X.rows_written(m, "rows_past_m") > m for m in ms) >= 5      # every M that is no multiple of the tile writes into the guard
