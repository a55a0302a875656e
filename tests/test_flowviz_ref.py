"""CPU: the restatement of flow2color and of the flow error measures (flowviz_ref.py) against known answers.

tests/test_gpu_flowviz.py compares the GPU with the restatement; here the restatement itself is pinned: the hue wheel at its
cardinal and pure-colour directions, the white rule, MATLAB's max, the frame's maximum, the paste offset, hand-made error pairs and
the Yosemite flow's mean endpoint error as tests/test_yosemite.py computes it."""
import math

import numpy as np

import flowviz_ref as fr

F32, F64 = np.float32, np.float64
S3 = math.sqrt(3.0) / 2.0


def _one(u, v, maxvalue=None):
    img, m = fr.flow2color(np.array([[u]], F32), np.array([[v]], F32), maxvalue=maxvalue)
    return [float(x) for x in img[0, 0, :]], m


def test_cardinal_flows_give_quarter_hues():
    # atan2 of the exact arguments (0, 1), (1, 0), (0, -1), (-1, 0) is 0, pi/2, pi, -pi/2 to the last bit: exact colours
    assert _one(-1, 0) == ([1.0, 0.0, 0.0], 1.0)        # hue 0: red
    assert _one(0, -1) == ([0.5, 1.0, 0.0], 1.0)        # hue 1/4
    assert _one(1, 0) == ([0.0, 1.0, 1.0], 1.0)         # hue 1/2: cyan
    assert _one(0, 1) == ([0.5, 0.0, 1.0], 1.0)         # hue 3/4


def test_pure_colour_flows():
    """The six directions whose hue is a multiple of 1/6.  sqrt(3)/2 is rounded to float32 on the way in: the components are off by
    at most 2^-25 relative, so is the magnitude (below 1 after dividing by 1), the hue by at most 2^-25 / (2 pi) turns and the sector
    fraction by six times that; 2^-22 bounds all of it."""
    want = {(-1.0, 0.0): (1.0, 0.0, 0.0), (-0.5, -S3): (1.0, 1.0, 0.0), (0.5, -S3): (0.0, 1.0, 0.0), (1.0, 0.0): (0.0, 1.0, 1.0),
            (0.5, S3): (0.0, 0.0, 1.0), (-0.5, S3): (1.0, 0.0, 1.0)}
    for (u, v), rgb in want.items():
        got, _ = _one(u, v, maxvalue=1.0)
        assert np.max(np.abs(np.array(got) - np.array(rgb))) <= 2.0 ** -22, ((u, v), got)


def test_half_magnitude_gives_half_value():
    assert _one(-0.5, 0, maxvalue=1.0)[0] == [0.5, 0.0, 0.0]
    assert _one(0.5, 0, maxvalue=1.0)[0] == [0.0, 0.5, 0.5]
    assert _one(0, -1, maxvalue=2.0)[0] == [0.25, 0.5, 0.0]
    assert _one(3, 0, maxvalue=2.0)[0] == [0.0, 1.0, 1.0]   # clamped at 1


def test_invalid_pixels_are_white():
    white = [1.0, 1.0, 1.0]
    assert _one(math.nan, 1.0, maxvalue=1.0)[0] == white
    assert _one(1.0, math.nan, maxvalue=1.0)[0] == white
    assert _one(math.inf, 0.0, maxvalue=1.0)[0] == white
    assert _one(-math.inf, 0.0, maxvalue=1.0)[0] == white
    # the .m tests isfinite on U alone: an Inf in V clamps to full magnitude and keeps its direction (hue 1/4 or 3/4)
    assert _one(0.0, -math.inf, maxvalue=1.0)[0] == [0.5, 1.0, 0.0]


def test_inf_under_the_automatic_max_blackens_the_rest():
    U = np.array([[1.0, math.inf], [-2.0, 0.5]], F32)
    V = np.array([[1.0, 0.0], [0.0, -0.5]], F32)
    img, m = fr.flow2color(U, V)
    assert m == math.inf
    assert np.array_equal(img[0, 1, :], [1, 1, 1])   # Inf / Inf is NaN: white
    for i, j in ((0, 0), (1, 0), (1, 1)):
        assert np.array_equal(img[i, j, :], [0, 0, 0])   # finite / Inf is 0: black


def test_max_ignores_nan_and_zero_and_all_nan_fields_are_white():
    U = np.array([[math.nan, 3.0, 1.0]], F32)
    V = np.array([[9.0, 4.0, math.nan]], F32)
    assert fr.max_magnitude(U, V) == 5.0
    img, m = fr.flow2color(np.zeros((3, 4), F32), np.zeros((3, 4), F32))
    assert m == 0.0 and np.all(img == 1.0)   # 0 / 0
    img, m = fr.flow2color(np.full((3, 4), np.nan, F32), np.full((3, 4), np.nan, F32))
    assert math.isnan(m) and np.all(img == 1.0)
    z = np.array([[-0.0, 0.0]], F32)
    img, m = fr.flow2color(z, z[:, ::-1], maxvalue=1.0)
    assert np.all(img == 0.0)   # zero magnitude is black whatever the zero's sign


def test_frame_maximum_is_sqrt_50_at_the_last_pixel():
    for brows, bcols in ((3, 3), (39, 55), (57, 73), (300, 7)):
        X, Y = fr.frame_field(brows, bcols)
        mag = np.sqrt(X * X + Y * Y)
        assert mag.max() == math.sqrt(50.0) == mag[-1, -1] and X[-1, -1] == 5.0 == Y[-1, -1]
        assert int(np.argmax(mag)) == mag.size - 1 and (mag == mag.max()).sum() == 1


def test_paste_offset_is_border_minus_one():
    rng = np.random.default_rng(3)
    U, V = rng.normal(size=(5, 7)).astype(F32), rng.normal(size=(5, 7)).astype(F32)
    plain, m0 = fr.flow2color(U, V)
    for border in (1, 2, 10):
        img, m = fr.flow2color(U, V, border=border)
        assert img.shape == (5 + 2 * border, 7 + 2 * border, 3) and m == m0
        o = border - 1
        assert np.array_equal(img[o:o + 5, o:o + 7, :], plain)
        # everything else is the frame: the colour coding of the synthetic field alone
        X, Y = fr.frame_field(*img.shape[:2])
        frame, fm = fr.flow2color(X.astype(F32), Y.astype(F32))
        rest = np.ones(img.shape[:2], bool)
        rest[o:o + 5, o:o + 7] = False
        assert fm == math.sqrt(50.0)
        # (the frame is computed from the float64 field, `frame` from its float32 rounding: close, not equal)
        assert np.max(np.abs(img[rest] - frame[rest])) < 1e-5
        # the last pixel is the frame's (5, 5): hue 5/8 at full value, sector 3 with f = 3/4
        assert np.max(np.abs(img[-1, -1, :] - np.array([0.0, 0.25, 1.0]))) < 1e-6


def test_uint8_rounding_is_half_away_from_zero():
    x = np.array([0.0, 0.5 / 255, 1.5 / 255, 0.4999 / 255, 1.0, 254.5 / 255, 0.25], F64).astype(F32)
    y = 255.0 * x.astype(F64)
    want = [0 if v < 0.5 else int(math.floor(v + 0.5)) for v in y]
    assert list(fr.to_uint8(x)) == want
    assert fr.to_uint8(np.array([1.0], F32))[0] == 255 and fr.to_uint8(np.array([0.5], F32))[0] == 128   # 127.5 rounds up
    img = np.zeros((2, 3, 3), F32)
    img[1, 2, 0] = 1.0
    flat = fr.to_uint8(img).tobytes()
    assert flat[(1 * 3 + 2) * 3 + 0] == 255 and sum(flat) == 255   # row-major, interleaved


def test_error_measures_of_hand_made_pairs():
    rng = np.random.default_rng(5)
    U, V = rng.normal(size=(4, 6)).astype(F32), rng.normal(size=(4, 6)).astype(F32)
    e = fr.flow_errors(U, V, U, V)
    assert e["count"] == 24 and e["mean_epe"] == 0.0 and e["max_epe"] == 0.0 and not e["epe"].any()
    # identical fields: the cosine is 1 up to rounding, clamped; acos amplifies one ulp below 1 to sqrt(2 * 2^-53) rad
    assert e["mean_ang"] <= math.degrees(math.sqrt(2.0 ** -52)) and np.all(e["ang"] >= 0)
    one, zero = np.ones((1, 1), F32), np.zeros((1, 1), F32)
    e = fr.flow_errors(one, zero, -one, zero)   # opposite unit flows: (1, 0, 1) against (-1, 0, 1)
    assert e["mean_epe"] == 2.0 == e["max_epe"]
    assert e["mean_ang"] == math.acos(0.0 / (math.sqrt(2.0) * math.sqrt(2.0))) * (180.0 / math.pi) == 90.0
    e = fr.flow_errors(zero, zero, one, zero)   # (0, 0, 1) against (1, 0, 1): 45 degrees, endpoint error 1
    assert e["mean_epe"] == 1.0 and abs(e["mean_ang"] - 45.0) < 1e-13
    e = fr.flow_errors(3 * one, 4 * one, zero, zero)
    assert e["mean_epe"] == 5.0 and abs(e["mean_ang"] - math.degrees(math.acos(1.0 / math.sqrt(26.0)))) < 1e-13


def test_error_measures_exclude_masked_and_nonfinite_pixels():
    U = np.array([[1.0, math.nan, 2.0, 0.0], [0.0, 1.0, math.inf, 3.0]], F32)
    V = np.zeros((2, 4), F32)
    Ut = np.zeros((2, 4), F32)
    Vt = np.array([[0.0, 0.0, 0.0, math.nan], [0.0, 0.0, 0.0, 4.0]], F32)
    mask = np.array([[1.0, 1.0, 0.0, 1.0], [-2.0, 1.0, 1.0, 1.0]], F32)
    e = fr.flow_errors(U, V, Ut, Vt, mask)
    want = np.array([[True, False, False, False], [True, True, False, True]])
    assert np.array_equal(e["counted"], want) and e["count"] == 4
    assert np.array_equal(np.isnan(e["epe"]), ~want) and np.array_equal(np.isnan(e["ang"]), ~want)
    assert e["max_epe"] == 5.0 and e["mean_epe"] == (1.0 + 0.0 + 1.0 + 5.0) / 4
    e = fr.flow_errors(U, V, Ut, Vt, np.zeros((2, 4), F32))
    assert e["count"] == 0 and math.isnan(e["mean_epe"]) and math.isnan(e["mean_ang"]) and math.isnan(e["max_epe"])


def test_yosemite_mean_endpoint_error_is_that_of_test_yosemite(oracle):
    """Same fields, same per-pixel float64 operations, another summation order: n * 2^-53 relative.  _errors() is handed the float32
    fields promoted to float64 (exactly): on float32 arrays it does its arithmetic in float32, which is 8e-8 from any float64
    evaluation and no statement about the summation."""
    import test_yosemite as ty

    U, V = ty.statement_flow(oracle)
    _, _, Ut, Vt = ty._data()
    assert U.dtype == F32 and Ut.dtype == F32
    want_all, want_land = ty._errors(*[a.astype(F64) for a in (U, V, Ut, Vt)])
    tol = U.size * 2.0 ** -53
    e = fr.flow_errors(U, V, Ut, Vt)
    print("all pixels: restatement %.17g, _errors %.17g, relative difference %.3g (bound %.3g)"
          % (e["mean_epe"], want_all, abs(e["mean_epe"] - want_all) / want_all, tol))
    assert e["count"] == U.size and abs(e["mean_epe"] - want_all) <= tol * want_all
    mask = np.zeros(U.shape, F32)
    mask[90:, :] = 1.0
    e = fr.flow_errors(U, V, Ut, Vt, mask)
    assert e["count"] == (U.shape[0] - 90) * U.shape[1] and abs(e["mean_epe"] - want_land) <= tol * want_land
    assert e["mean_epe"] < 0.2
