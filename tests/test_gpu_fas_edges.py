"""GPU: the nine stage kernels of the FAS full-multigrid flow driver (csrc/pdeip_fas.hpp) at workgroup seams, partial prepare tiles,
the smallest planes, resize ratios the driver never uses, non-finite / signed-zero / subnormal data and aliased arguments, bit for bit
against the numpy statement (oracle/matlab_side.py fas_*).  The cases come from tests/fas_edge_cases.py; tests/test_fas_edge_cases.py
proves on the CPU what each of them contains.

Every comparison is problems.bit_equal: bits equal (those of zeros too), any NaN equals any NaN.  No tolerance anywhere."""
import functools

import numpy as np
import pytest

import fas_edge_cases as fc
import problems as pb
from test_gpu_flow_level import matlab_side, same, sub

pytestmark = pytest.mark.gpu
F32 = np.float32
SENTINEL = -7.0
SUMMED = ("M", "Cu", "Cv", "Du", "Dv")


@functools.lru_cache(maxsize=None)
def ms():
    return matlab_side()


def up(a):
    """A case on the device (the cases are read-only; torch wants a writable array to wrap)."""
    return sub("device").to_device(np.array(a, dtype=F32, order="F"))


def quiet(fn, *args):
    with np.errstate(invalid="ignore", over="ignore", divide="ignore", under="ignore"):
        return fn(*args)


def c3(a):
    return a if a.ndim == 3 else a[:, :, None]


def same3(got, want, what):
    """A [rows, cols, C] stack; the device hands a one-channel stack back as it got it."""
    same(c3(np.asarray(got)), c3(np.asarray(want)), what)


@functools.lru_cache(maxsize=None)
def want_planes(shape):
    return ms().fas_prepare(*fc.frames(shape), fc.B1, fc.B2)


@functools.lru_cache(maxsize=None)
def dev_planes(shape):
    """The statement's planes on the device as one [13, C, ncols, nrows] block: what the assembly reads does not depend on
    k_fas_prepare being right."""
    import torch
    want = want_planes(shape)
    return torch.stack([up(want[name]).reshape(fc.channels(shape), shape[1], shape[0]) for name in ms().FAS_PLANES]).contiguous()


def stack_like(planes):
    import torch
    return torch.empty_like(planes[0])


def products(want, gd, names=SUMMED):
    return {n: quiet(lambda a, b: (a * b).astype(F32), want[n], gd) for n in names}


# ---- per shape, against the statement --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", fc.SHAPES, ids=fc.tag)
def test_gauss5_and_down(pdeip, shape):
    dev = sub("device")
    I0, _ = fc.frames(shape)
    G = ms().fas_gaussian5(1.0)
    g0 = dev.fas_gauss5(up(I0), G)
    w0 = ms().fas_gauss5(I0, G)
    same3(dev.to_matlab(g0), w0, "gauss5 %s" % (shape,))
    down = dev.fas_down(g0)
    assert tuple(down.shape[-2:]) == fc.coarse(shape)[::-1]
    same3(dev.to_matlab(down), ms().fas_down(w0), "down of gauss5 %s" % (shape,))
    same3(dev.to_matlab(dev.fas_down(up(I0))), ms().fas_down(I0), "down of the noise itself %s" % (shape,))


@pytest.mark.parametrize("shape", fc.SHAPES, ids=fc.tag)
def test_prepare_all_thirteen_planes(pdeip, shape):
    dev = sub("device")
    I0, I1 = fc.frames(shape)
    planes = dev.fas_prepare(up(I0), up(I1), fc.B1, fc.B2)
    assert tuple(planes.shape) == (13, fc.channels(shape), shape[1], shape[0])
    want = want_planes(shape)
    for k, name in enumerate(ms().FAS_PLANES):
        same3(dev.to_matlab(planes[k]), want[name], "prepare %s %s" % (name, shape))


@pytest.mark.parametrize("shape", fc.SHAPES, ids=fc.tag)
def test_restrict_and_rhs(pdeip, shape):
    dev = sub("device")
    I0, _ = fc.frames(shape)
    f, want = fc.fields(shape), want_planes(shape)
    for scale in (0.5, 1.0):
        same(dev.to_matlab(dev.fas_restrict(up(f["U"]), scale)), ms().fas_restrict(f["U"], scale), "restrict plane %s x%g" % (shape, scale))
        same3(dev.to_matlab(dev.fas_restrict(up(I0), scale)), ms().fas_restrict(I0, scale), "restrict stack %s x%g" % (shape, scale))
    gd = ms().fas_gd(want, f["U"], f["V"], fc.B1, fc.B2, fc.ALPHA)
    got = dev.fas_rhs(up(want["Du"]), up(f["A"]), up(gd))
    same3(dev.to_matlab(got), ((want["Du"] + c3(f["A"])) / gd).astype(F32), "rhs %s" % (shape,))


@pytest.mark.parametrize("shape", fc.SHAPES, ids=fc.tag)
def test_assemble_per_frame_forms(pdeip, shape):
    """The form of the cycle's coarse step (Cu = Cv = NULL, gd wanted: pdeip_drivers.hip, fas.py cycle()) leaves the CuGd / CvGd
    buffers alone; the residual's form (Cu, Cv given, gd = None) writes all five."""
    import torch
    dev, fas = sub("device"), sub("fas")
    f, want, planes = fc.fields(shape), want_planes(shape), dev_planes(shape)
    dU, dV = up(f["U"]), up(f["V"])
    gd = ms().fas_gd(want, f["U"], f["V"], fc.B1, fc.B2, fc.ALPHA)
    prod = products(want, gd)
    M, Du, Dv, g = [stack_like(planes) for _ in range(4)]
    cu, cv = torch.full_like(planes[0], SENTINEL), torch.full_like(planes[0], SENTINEL)
    dev.fas_assemble(planes, None, None, dU, dV, fc.B1, fc.B2, fc.ALPHA, True, M, cu, cv, Du, Dv, g)
    for t, name in ((M, "M"), (Du, "Du"), (Dv, "Dv")):
        same3(dev.to_matlab(t), prod[name], "per-frame %s.*gd, no right-hand side %s" % (name, shape))
    same3(dev.to_matlab(g), gd, "gd %s" % (shape,))
    assert bool((cu == SENTINEL).all()) and bool((cv == SENTINEL).all()), "CuGd / CvGd written without a Cu / Cv"
    per = [stack_like(planes) for _ in range(5)]
    dev.fas_assemble(planes, planes[fas.CU], planes[fas.CV], dU, dV, fc.B1, fc.B2, fc.ALPHA, True, *per)
    for t, name in zip(per, SUMMED):
        same3(dev.to_matlab(t), prod[name], "per-frame %s.*gd, gd = None %s" % (name, shape))


def run_summed(dev, planes, Cu, Cv, dU, dV, k):
    import torch
    one = [torch.empty_like(dU) for _ in range(5)]
    dev.fas_assemble(planes, Cu, Cv, dU, dV, fc.B1, fc.B2, k, False, *one)
    return [dev.to_matlab(t) for t in one]


def run_weights_form(dev, planes, Cu, Cv, dU, dV, k):
    import torch
    out = [torch.empty_like(dU) for _ in range(9)]
    dev.fas_assemble_weights(planes, Cu, Cv, dU, dV, fc.B1, fc.B2, k, *out)
    return [dev.to_matlab(t) for t in out]


def check_weights_form(dev, planes, want, U, V, k, what):
    """pdeip_fas_assemble_weights_dev == pdeip_fas_assemble_dev(per_frame = 0) + pdeip_flow_opdiffweights_dev(U, V), byte for byte, and
    both equal the statement."""
    import torch
    fas = sub("fas")
    dU, dV = up(U), up(V)
    fused = run_weights_form(dev, planes, planes[fas.CU], planes[fas.CV], dU, dV, k)
    summed = run_summed(dev, planes, planes[fas.CU], planes[fas.CV], dU, dV, k)
    w4 = [torch.empty_like(dU) for _ in range(4)]
    dev.flow_opdiffweights(dU, dV, None, None, *w4)
    apart = summed + [dev.to_matlab(t) for t in w4]
    gd = quiet(ms().fas_gd, want, U, V, fc.B1, fc.B2, k)
    zero = np.zeros(U.shape, F32)
    stated = [quiet(ms()._sum3, quiet(np.multiply, want[n], gd)) for n in SUMMED] + list(quiet(ms().op_diff_weights, U, V, zero, zero))
    for name, a, b, c in zip(SUMMED + ("wW", "wN", "wS", "wE"), fused, apart, stated):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), "%s: fused %s differs from the two launches" % (what, name)
        same(a, c, "%s: fused %s" % (what, name))
        same(b, c, "%s: %s of the two launches" % (what, name))
    return stated


@pytest.mark.parametrize("shape", fc.SHAPES, ids=fc.tag)
def test_assemble_weights_equals_the_two_launches_and_the_statement(pdeip, shape):
    f = fc.fields(shape)
    check_weights_form(sub("device"), dev_planes(shape), want_planes(shape), f["U"], f["V"], fc.channels(shape) * fc.ALPHA, "%s" % (shape,))


@pytest.mark.parametrize("shape", fc.SHAPES, ids=fc.tag)
def test_prolong_add(pdeip, shape):
    dev = sub("device")
    f = fc.fields(shape)
    got = up(f["U"])
    dev.fas_prolong_add(got, up(f["Uc"]), up(f["Ur"]), 2.0)
    same(dev.to_matlab(got), ms().fas_prolong_add(f["U"], f["Uc"], f["Ur"], 2.0), "prolongation %s -> %s" % (fc.coarse(shape), shape))
    # equal sizes: the weights are 1 and 0, so U + (Uc - Ures) * inv_scale itself
    got = up(f["Uc"])
    dev.fas_prolong_add(got, up(f["Uc"]), up(f["Ur"]), 2.0)
    want = (f["Uc"] + ((f["Uc"] - f["Ur"]) * F32(2.0)).astype(F32)).astype(F32)
    same(dev.to_matlab(got), want, "prolongation at equal sizes %s" % (fc.coarse(shape),))


@pytest.mark.parametrize("shape", fc.SHAPES, ids=fc.tag)
def test_upscale_ratios(pdeip, shape):
    dev = sub("device")
    Uc = fc.fields(shape)["Uc"]
    d = up(Uc)
    for out in fc.upscale_targets(shape):
        got = dev.to_matlab(dev.fas_upscale(d, 2.0, *out))
        same(got, ms().fas_upscale(Uc, 2.0, *out), "bicubic upscale %s -> %s" % (Uc.shape, out))
        if out == Uc.shape:
            same(got, (Uc * F32(2.0)).astype(F32), "upscale to equal size is in * mul")


@pytest.mark.parametrize("shape", fc.TAIL_SHAPES, ids=fc.tag)
def test_no_write_past_the_end_and_every_output_written(pdeip, shape):
    """The C entries themselves, the output followed by 64 floats of sentinel: the tail comes back untouched, and of the NaN the output
    was filled with none is left (a grid sized by the wrong row count leaves pixels unwritten or writes beyond)."""
    import torch
    dev, capi = sub("device"), pdeip.capi
    I0, _ = fc.frames(shape)
    C, (cr, cc) = fc.channels(shape), fc.coarse(shape)
    Uc = fc.fields(shape)["Uc"]
    dI, dUc = up(I0), up(Uc)

    def run(n, want, what, name, *args):
        buf = torch.full((n + fc.TAIL,), float("nan"), device="cuda")
        buf[n:] = SENTINEL
        capi.call(name, dev._stream(), *[buf.data_ptr() if a is None else a for a in args])
        torch.cuda.synchronize()
        got = buf.cpu().numpy()
        assert bool((got[n:] == F32(SENTINEL)).all()), "%s wrote past the end" % what
        assert not np.isnan(want).any()
        want = np.asarray(want, dtype=F32)
        flat = (want.transpose(2, 1, 0) if want.ndim == 3 else want.T).reshape(-1)     # the device layout: [C][ncols][nrows]
        same(got[:n], flat, what)

    run(C * cr * cc, ms().fas_down(I0), "down %s" % (shape,), "pdeip_fas_down_dev", dI.data_ptr(), shape[0], shape[1], C, None)
    run(C * cr * cc, c3(ms().fas_restrict(I0, 0.5)), "restrict %s" % (shape,), "pdeip_fas_restrict_dev", dI.data_ptr(), shape[0], shape[1], C, 0.5, None)
    for out in fc.upscale_targets(shape):
        run(out[0] * out[1], ms().fas_upscale(Uc, 2.0, *out), "upscale %s -> %s" % ((cr, cc), out), "pdeip_fas_upscale_dev", dUc.data_ptr(), cr, cc, 2.0,
            out[0], out[1], None)


# ---- the order of the frame sum ----------------------------------------------------------------------------------------------------------

def test_frames_are_summed_first_to_last(pdeip):
    """Five frames whose gd differ by orders of magnitude: summing last to first changes bits at a third of the pixels (proved on the
    CPU), so the forward order of sum(.,3) is pinned, in the plain and in the fused form."""
    dev, fas = sub("device"), sub("fas")
    I0, I1 = fc.order_frames()
    f = fc.fields(fc.ORDER_SHAPE)
    want = ms().fas_prepare(I0, I1, fc.B1, fc.B2)
    planes = dev.fas_prepare(up(I0), up(I1), fc.B1, fc.B2)
    for k, name in enumerate(ms().FAS_PLANES):
        same3(dev.to_matlab(planes[k]), want[name], "prepare %s of the order case" % name)
    k = fc.ORDER_C * fc.ALPHA
    gd = ms().fas_gd(want, f["U"], f["V"], fc.B1, fc.B2, k)
    dU, dV = up(f["U"]), up(f["V"])
    for form, got in (("summed", run_summed(dev, planes, planes[fas.CU], planes[fas.CV], dU, dV, k)),
                      ("fused", run_weights_form(dev, planes, planes[fas.CU], planes[fas.CV], dU, dV, k)[:5])):
        for g, name in zip(got, SUMMED):
            P = want[name] * gd
            assert not pb.bit_equal(ms()._sum3(P), fc.sum3_reversed(P))
            same(g, ms()._sum3(P), "%s sum(%s.*gd, 3), first frame first" % (form, name))


# ---- values --------------------------------------------------------------------------------------------------------------------------------

def check_image_stages(dev, I0, I1, what, G=None):
    """gauss5, down, restrict and prepare of a frame pair, every plane whole: NaN and Inf footprints follow from the bits."""
    G = ms().fas_gaussian5(1.0) if G is None else G
    for k, I in enumerate((I0, I1)):
        g = dev.fas_gauss5(up(I), G)
        w = quiet(ms().fas_gauss5, I, G)
        same3(dev.to_matlab(g), w, "%s: gauss5, frame %d" % (what, k))
        same3(dev.to_matlab(dev.fas_down(g)), quiet(ms().fas_down, w), "%s: down of gauss5, frame %d" % (what, k))
        same3(dev.to_matlab(dev.fas_down(up(I))), quiet(ms().fas_down, I), "%s: down, frame %d" % (what, k))
        for scale in (0.5, 1.0):
            same3(dev.to_matlab(dev.fas_restrict(up(I), scale)), quiet(ms().fas_restrict, I, scale), "%s: restrict x%g, frame %d" % (what, scale, k))
    planes = dev.fas_prepare(up(I0), up(I1), fc.B1, fc.B2)
    want = quiet(ms().fas_prepare, I0, I1, fc.B1, fc.B2)
    for k, name in enumerate(ms().FAS_PLANES):
        same3(dev.to_matlab(planes[k]), want[name], "%s: prepare %s" % (what, name))
    return want


@pytest.mark.parametrize("where", ["interior", "corners"])
def test_nan_and_inf_pixels(pdeip, where):
    """One NaN, one +Inf and one -Inf pixel: 25 NaN under gauss5; under prepare the zero centre tap of the derivative kernel turns the
    middle of an Inf footprint into NaN (0 * Inf), and Inf - Inf makes Cu, Cv NaN.  In the corners the clamp cuts the footprints."""
    dev = sub("device")
    I0, I1 = fc.nonfinite_frames(where)
    want = check_image_stages(dev, I0, I1, where)
    if where == "interior":
        assert {k: fc.footprint(v) for k, v in want.items()} == {k: fc.FOOTPRINTS[where][k] for k in ms().FAS_PLANES}


def test_gauss5_multiplies_by_its_zero_taps(pdeip):
    """fspecial('gaussian', [5 5], 0.15) has 20 taps that are exactly zero; an Inf pixel under them is 0 * Inf = NaN."""
    dev = sub("device")
    G = ms().fas_gaussian5(0.15)
    I0, _ = fc.nonfinite_frames("posinf")
    want = quiet(ms().fas_gauss5, I0, G)
    assert fc.footprint(want) == (20, 5)
    same3(dev.to_matlab(dev.fas_gauss5(up(I0), G)), want, "gauss5 with zero taps over an Inf pixel")
    clean, _ = fc.nonfinite_frames("clean")
    same3(dev.to_matlab(dev.fas_gauss5(up(clean), G)), ms().fas_gauss5(clean, G), "gauss5 with zero taps over numbers")


def test_signed_zeros(pdeip):
    """A plane of -0.0: -0.0 after gauss5, down, restrict and the prolongation (first terms are taken, not added to +0), +0.0 after a
    bicubic enlargement (negative weights), -0.0 after one to equal size."""
    dev = sub("device")
    cs = fc.coarse(fc.VALUE_SHAPE)
    mz, mzc, pzc = np.full(fc.VALUE_SHAPE, -0.0, F32), np.full(cs, -0.0, F32), np.zeros(cs, F32)
    G = ms().fas_gaussian5(1.0)
    minus = lambda shape: np.full(shape, -0.0, F32)
    same(dev.to_matlab(dev.fas_gauss5(up(mz), G)), minus(fc.VALUE_SHAPE), "gauss5 of -0")
    same(dev.to_matlab(dev.fas_down(up(mz))), minus(cs), "down of -0")
    same(dev.to_matlab(dev.fas_restrict(up(mz), 0.5)), minus(cs), "restrict of -0")
    for Ures, want in ((pzc, minus(fc.VALUE_SHAPE)), (mzc, np.zeros(fc.VALUE_SHAPE, F32))):
        got = up(mz)
        dev.fas_prolong_add(got, up(mzc), up(Ures), 2.0)
        same(dev.to_matlab(got), want, "prolongation of -0 (Ures %s0)" % ("-" if np.signbit(Ures[0, 0]) else "+"))
        same(want, ms().fas_prolong_add(mz, mzc, Ures, 2.0), "the statement")
    same(dev.to_matlab(dev.fas_upscale(up(mzc), 2.0, *fc.VALUE_SHAPE)), np.zeros(fc.VALUE_SHAPE, F32), "upscale of -0: +0")
    same(dev.to_matlab(dev.fas_upscale(up(mzc), 2.0, *cs)), minus(cs), "upscale of -0 to equal size: -0")
    same(ms().fas_upscale(mzc, 2.0, *fc.VALUE_SHAPE), np.zeros(fc.VALUE_SHAPE, F32), "the statement")


@pytest.mark.parametrize("scale", fc.SUBNORMAL_SCALES)
def test_subnormals_are_not_flushed(pdeip, scale):
    """Frames times 1e-41: subnormal frames and derivative planes, products that underflow to zero; times 1e-20: subnormal products."""
    dev = sub("device")
    I0, I1 = fc.subnormal_frames(scale)
    want = check_image_stages(dev, I0, I1, "frames x %g" % scale)
    assert any(fc.subnormal(want[name]).any() for name in ms().FAS_PLANES)


def check_assemble_values(dev, U, V, k, what):
    """Both per-frame forms and the summed one on the 'clean' planes of the value cases, at a flow and a k that overflow or divide by 0."""
    import torch
    fas = sub("fas")
    v = fc.value_fields()
    want = v["planes"]
    planes = torch.stack([up(want[name]) for name in ms().FAS_PLANES]).contiguous()
    dU, dV = up(U), up(V)
    gd = quiet(ms().fas_gd, want, U, V, fc.B1, fc.B2, k)
    prod = products(want, gd)
    per = [stack_like(planes) for _ in range(6)]
    dev.fas_assemble(planes, planes[fas.CU], planes[fas.CV], dU, dV, fc.B1, fc.B2, k, True, *per)
    for t, name in zip(per[:5], SUMMED):
        same3(dev.to_matlab(t), prod[name], "%s: per-frame %s.*gd" % (what, name))
    same3(dev.to_matlab(per[5]), gd, "%s: gd" % what)
    check_weights_form(dev, planes, want, U, V, k, what)
    return gd, per[5]


def test_overflowing_opnorm_and_zero_k(pdeip):
    """U = 1e20: OPnorm overflows at some pixels and gd is +0 there, so the products are zeros of both signs (the first frame of the sum
    is taken, not added to +0).  k = 0: gd is Inf everywhere and the sum over the frames Inf - Inf.  Both gd as divisors of the
    right-hand side: x/0, 0/0, x/Inf."""
    dev = sub("device")
    v = fc.value_fields()
    gd, d_huge = check_assemble_values(dev, v["Uhuge"], v["V"], fc.ALPHA, "U = 1e20")
    assert pb.bit_equal(gd, v["gd_huge"]) and bool((gd == 0).any())
    gd, d_k0 = check_assemble_values(dev, v["U"], v["V"], 0.0, "k = 0")
    assert pb.bit_equal(gd, v["gd_k0"]) and bool((gd == np.inf).all())
    dR, dA = up(v["R"]), up(v["A"])
    s = (v["R"] + v["A"]).astype(F32)
    for what, d_gd, gd in (("x/0 and 0/0", d_huge, v["gd_huge"]), ("x/Inf", d_k0, v["gd_k0"])):
        want = quiet(np.divide, s, gd).astype(F32)
        same3(dev.to_matlab(dev.fas_rhs(dR, dA, d_gd)), want, "rhs, %s" % what)
        same3(dev.to_matlab(dev.fas_rhs(dR, dA, up(gd))), want, "rhs, %s (the statement's gd)" % what)


def test_one_nan_in_the_flow(pdeip):
    """Per frame the NaN stays at its pixel; in the fused form the weights carry it to the neighbours exactly as OPdiffWeights says."""
    dev = sub("device")
    v = fc.value_fields()
    gd, _ = check_assemble_values(dev, v["Unan"], v["V"], fc.ALPHA, "one NaN in U")
    assert int(np.isnan(gd).sum()) == fc.VALUE_C


# ---- aliased arguments -------------------------------------------------------------------------------------------------------------------

def test_halving_and_upscale_refuse_an_aliased_output(pdeip):
    import torch
    dev, capi = sub("device"), pdeip.capi
    I = up(fc.frames((64, 4))[0])
    before = I.clone()
    p = I.data_ptr()
    for name, args in (("pdeip_fas_down_dev", (p, 64, 4, 1, p)), ("pdeip_fas_restrict_dev", (p, 64, 4, 1, 0.5, p)),
                       ("pdeip_fas_upscale_dev", (p, 64, 4, 2.0, 64, 4, p)), ("pdeip_fas_gauss5_dev", (p, 64, 4, 1, ms().fas_gaussian5(1.0).ctypes.data, p))):
        with pytest.raises(capi.PdeipError) as e:
            capi.call(name, dev._stream(), *args)
        assert e.value.code == capi.PDEIP_ERR_ARG
        assert name in str(e.value) and name in capi.last_error() and "alias" in capi.last_error()
    torch.cuda.synchronize()
    assert torch.equal(I, before)


def test_resizing_stages_admit_what_a_side_of_three_halves_to(pdeip):
    """down and restrict turn a side of 3 into 2, so the prolongation and the bicubic upscale take planes from 2 x 2 on (the MIN
    shapes run them against the statement); a side of 1 is refused and nothing is written."""
    import torch
    dev, capi = sub("device"), pdeip.capi
    for shape in ((1, 5), (5, 1)):
        small = torch.full(shape[::-1], 1.0, device="cuda")
        big = torch.full((6, 6), SENTINEL, device="cuda")
        with pytest.raises(capi.PdeipError) as e:
            dev.fas_prolong_add(big, small, small, 2.0)
        assert e.value.code == capi.PDEIP_ERR_ARG and "pdeip_fas_prolong_add_dev" in str(e.value) and "at least 2x2" in str(e.value)
        with pytest.raises(capi.PdeipError) as e:
            capi.call("pdeip_fas_upscale_dev", dev._stream(), small.data_ptr(), shape[0], shape[1], 2.0, 6, 6, big.data_ptr())
        assert e.value.code == capi.PDEIP_ERR_ARG and "pdeip_fas_upscale_dev" in str(e.value) and "at least 2x2" in str(e.value)
        torch.cuda.synchronize()
        assert bool((big == SENTINEL).all())


def test_rhs_in_place_equals_out_of_place(pdeip):
    """Elementwise, so out == R is allowed."""
    import torch
    dev, capi = sub("device"), pdeip.capi
    shape = (257, 3)
    f, want = fc.fields(shape), want_planes(shape)
    gd = ms().fas_gd(want, f["U"], f["V"], fc.B1, fc.B2, fc.ALPHA)
    R, A, g = up(want["Du"]), up(f["A"]), up(gd)
    apart = dev.fas_rhs(R, A, g)
    capi.call("pdeip_fas_rhs_dev", dev._stream(), R.data_ptr(), A.data_ptr(), g.data_ptr(), shape[0], shape[1], fc.channels(shape), R.data_ptr())
    torch.cuda.synchronize()
    assert torch.equal(R, apart)
    same3(dev.to_matlab(R), ((want["Du"] + f["A"]) / gd).astype(F32), "rhs in place")


# ---- one driver case across the seam -----------------------------------------------------------------------------------------------------

def test_driver_across_the_row_seam(pdeip, oracle):
    """259 x 23, 130 x 12, 65 x 6: the only place the prolongation 130 -> 259 and the restriction 259 -> 130 meet the real solver."""
    dev, fas, D = sub("device"), sub("fas"), sub("drivers")
    I0, I1 = fc.frames(fc.SEAM_DRIVER_SHAPE, fc.SEAM_DRIVER_C)
    param = dict(alpha=0.035, omega=1.9, firstLoop=1, iter=2, b1=0.03, b2=0.97, scl_factor=0.5, solver=2, cycle_index=2)
    wU, wV = ms().fas_fmg(oracle, I0, I1, dict(param, order=0))
    drv = fas.FasFmgFlow(param, mode=0)
    gU, gV = drv.run(up(I0), up(I1))
    assert [tuple(p.shape[-2:]) for p in drv.planes] == [(23, 259), (12, 130), (6, 65)]
    gU, gV = dev.to_matlab(gU), dev.to_matlab(gV)
    same(gU, wU, "driver U across the seam")
    same(gV, wV, "driver V across the seam")
    assert np.isfinite(wU).all() and np.abs(wU).max() > 1e-3
    cU, cV = D.capi_FlowEminNDFASFMG_elin_2D_v10(np.asfortranarray(np.concatenate([I0, I1], axis=2)), fc.SEAM_DRIVER_C, **param)
    same(cU, gU, "C driver U against the Python driver")
    same(cV, gV, "C driver V against the Python driver")
