"""CPU: the restatement of the hole filling (inpaint_ref.py) pinned against what the library already has -- matlab_side.tv4_assemble
and tv4_level without holes, pyramid.resize on a fully known plane -- and against closed-form answers at the ties; then its quality on
the 96 x 128 scene of inpaint_cases.py with the default parameters.

Measured with the oracle's solver (printed below): RMS error over the holes 3.11 px for the mean fill, 1.20 px inpainted without
the guide, 0.47 px with it; inside the occlusion band 2.13, 1.05 and 0.88 px."""
import numpy as np
import pytest

import inpaint_cases as ic
import inpaint_ref as ir
import problems as pb

F32, F64 = np.float32, np.float64


def same(got, want, what):
    assert pb.bit_equal(got, want), "%s: %s" % (what, pb.describe_mismatch(got, want))


def test_without_holes_the_assembly_is_tv4_assemble(oracle):
    ms = ir.matlab_side()
    for shape, F in (((37, 53), 1), ((40, 48), 3)):
        X, D, _ = ic.assemble_case(shape, F, 0, "none")
        got, want = ir.assemble(X, D, 5.0), ms.tv4_assemble(X, D, 5.0)
        same(got[0], want[0], "TRACE"); same(got[1], want[1], "B")
        for g, w in zip(got[2], want[2]):
            same(g, w, "weights")
    D, X0, _ = ic.level_case(2, False)
    full = np.asfortranarray(np.where(np.isnan(D), X0, D))
    p = dict(alpha=5.0, omega=1.75, outer_iter=2, inner_iter=5, solver=2, order=0)
    same(ir.level(oracle, full, X0, p), ms.tv4_level(oracle, full, X0, p), "one level without holes")


def test_nan_resize_of_a_known_plane_is_resize():
    for (shape, out) in ic.RESIZE_SHAPES:
        D = ic.holed(shape, "none")
        same(ir.nan_resize(D, out[0], out[1], 1e-9), ir.pyramid().resize(D, out[0], out[1]), "nan_resize %s" % (shape,))


def test_the_cover_tie_keeps_the_pixel():
    D = ic.tie_plane()
    known = (~np.isnan(D)).astype(F32)
    den = ir.pyramid().resize(known, 4, 4, out_dtype=F64)
    assert (den == 0.5).all()
    kept = ir.nan_resize(D, 4, 4, 0.5)
    assert not np.isnan(kept).any()
    assert np.isnan(ir.nan_resize(D, 4, 4, np.nextafter(0.5, 1.0))).all()
    # a kept pixel is the weighted mean of its known taps alone
    num = ir.pyramid().resize(np.where(np.isnan(D), F32(0), D), 4, 4, out_dtype=F64)
    same(kept, (num / 0.5).astype(F32), "tie")


def test_meanfill():
    empty = np.full((5, 7), np.nan, F32)
    assert ir.frame_mean(empty) == 0 and (ir.meanfill(empty) == 0).all()
    D = ic.single_known((5, 9))
    got = ir.meanfill(D)
    for f in range(2):
        assert (got[:, :, f] == F32(-1.5 + 4.0 * f)).all()
    D = ic.holed((37, 53), "random")
    got = ir.meanfill(D)
    known = ~np.isnan(D)
    assert got[known].tobytes() == D[known].tobytes()
    assert abs(float(got[~known][0]) - float(np.mean(D[known].astype(F64)))) < 1e-6


def test_merge_keeps_the_known_bits():
    D = np.array([[-0.0, np.nan, np.inf], [1e-45, np.nan, -np.inf], [3.0, 0.0, np.nan]], F32)
    X = np.full((3, 3), 7.0, F32)
    out, filled = ir.merge(X, D)
    known = ~np.isnan(D)
    assert out[known].tobytes() == D[known].tobytes() and np.signbit(out[0, 0])
    assert (out[~known] == 7.0).all() and np.array_equal(filled, (~known).astype(F32))


def test_assembly_on_holes():
    X, D, guide = ic.assemble_case((40, 48), 3, 3, "random")
    TRACE, B, ws = ir.assemble(X, D, 5.0, guide, 20.0)
    hole = np.isnan(D)
    assert np.array_equal(np.isnan(TRACE), hole) and (B[hole] == 0).all() and np.isfinite(B).all()
    for w in ws:
        assert np.isfinite(w).all() and (w >= 0).all()
    plain = ir.assemble(X, D, 5.0)[2]
    assert all((g <= p).all() for g, p in zip(ws, plain))    # a guide can only lower a weight: the maximum runs over more planes


@pytest.fixture(scope="module")
def scene_runs(oracle):
    truth, sparse, guide, band = ic.scene()
    return {name: ir.tv_inpaint4(oracle, sparse, g)[0] for name, g in (("plain", None), ("guided", guide))}


def test_quality_on_the_scene(scene_runs):
    truth, sparse, guide, band = ic.scene()
    hole = np.isnan(sparse)
    assert 0.12 < hole.mean() < 0.14
    mean_fill = ic.rms(ir.meanfill(sparse), truth, hole)
    plain, guided = ic.rms(scene_runs["plain"], truth, hole), ic.rms(scene_runs["guided"], truth, hole)
    print("scene: RMS over the holes: mean fill %.3f, inpainted %.3f, guided %.3f; inside the band: mean fill %.3f, inpainted %.3f, guided %.3f"
          % (mean_fill, plain, guided, ic.rms(ir.meanfill(sparse), truth, band), ic.rms(scene_runs["plain"], truth, band),
             ic.rms(scene_runs["guided"], truth, band)))
    assert guided < 0.5 * mean_fill
    assert plain < mean_fill


def test_outputs_are_finite_and_in_range(oracle, scene_runs):
    truth, sparse, guide, band = ic.scene()
    lo, hi = np.nanmin(sparse), np.nanmax(sparse)
    for name, out in scene_runs.items():
        assert np.isfinite(out).all(), name
        assert lo - 1e-3 <= out.min() and out.max() <= hi + 1e-3, name
        known = ~np.isnan(sparse)
        assert out[known].tobytes() == sparse[known].tobytes()
    D, X0, g = ic.level_case(2, True)
    for order, solver in ((0, 1), (1, 2)):
        p = dict(alpha=5.0, omega=1.75, outer_iter=2, inner_iter=5, solver=solver, order=order, guide_scale=20.0)
        assert np.isfinite(ir.level(oracle, D, X0, p, g)).all()
    for shape in ((37, 53), (5, 90)):
        for kind in ic.HOLE_KINDS:
            out, filled = ir.tv_inpaint4(oracle, ic.holed(shape, kind), outer_iter=2, min_size=4)
            assert np.isfinite(out).all(), (shape, kind)
            assert np.array_equal(filled, np.isnan(ic.holed(shape, kind)).astype(F32))
