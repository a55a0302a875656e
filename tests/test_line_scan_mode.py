"""CPU: PDEIP_MODE_LINE_SCAN through the library state calls, the Python constants and the environment knob (no compute calls)."""
import pytest

import test_capi_symbols as tcs


def test_the_constant_is_exported(pdeip):
    assert pdeip.capi.MODE_LINE_SCAN == 2 and pdeip.MODE_LINE_SCAN == 2
    assert "MODE_LINE_SCAN" in pdeip.__all__
    header = open(tcs.os.path.join(tcs.ROOT, "include", "pdeip.h")).read()
    assert tcs.re.search(r"#define\s+PDEIP_MODE_LINE_SCAN\s+2\b", header)


def test_set_mode_takes_line_scan_and_refuses_three(pdeip):
    capi = pdeip.capi
    try:
        pdeip.mex_api.set_mode(capi.MODE_LINE_SCAN)
        assert capi.get_mode() == 2
        for bad in (3, 4, -1):
            with pytest.raises(capi.PdeipError) as exc:
                capi.set_mode(bad)
            assert exc.value.code == capi.PDEIP_ERR_ARG and "unknown sweep ordering %d" % bad in str(exc.value)
            assert capi.get_mode() == 2  # a refused call changes nothing
    finally:
        capi.set_mode(capi.MODE_EXACT_ORDER)


def test_the_environment_selects_line_scan(pdeip):
    """What an unchanged MATLAB session sets before starting; pattern of
    test_environment_knobs_reach_the_library."""
    for spelling in ("line_scan", "LINE_SCAN", "linescan", "2"):
        assert tcs._child(tcs._READ_MODE % "", {"PDEIP_MODE": spelling}).startswith("2 "), spelling
    # an explicit call made before the first use wins over the environment, either way round
    assert tcs._child(tcs._READ_MODE % "capi.set_mode(0);", {"PDEIP_MODE": "line_scan"}).startswith("0 ")
    assert tcs._child(tcs._READ_MODE % "capi.set_mode(2);", {"PDEIP_MODE": "red_black"}).startswith("2 ")
    assert tcs._child(tcs._READ_MODE % "", {"PDEIP_MODE": "3"}).startswith("0 ")  # not understood: the default stays
