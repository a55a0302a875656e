"""A reader of pdeip_debug_plan_alr: the library's own launch plan of a line-relaxation call (csrc/pdeip_alr_plan.hpp) under the knobs
of the environment (sor_plan.knobs).  The entry makes no HIP call, so it needs no GPU."""
import ctypes
from collections import namedtuple

MODEL_ID = {"elin4": 0, "llin4": 1, "llin8": 2, "disp4": 3, "pde4": 4, "pde8": 5}  # PDEIP_PLAN_ALR_* of include/pdeip.h
FAMILY = {0: None, 1: "small", 2: "zebra", 3: "exact", 4: "scan"}
KERNEL = {0: None, 1: "k_alr_zebra3", 2: "k_alr_zebra3_pair", 3: "k_alr_lex", 4: "k_alr_lex global", 5: "k_alr_scan"}
INFO, PASS = 12, 20
EXACT, RED_BLACK, LINE_SCAN = 0, 1, 2
Plan = namedtuple("Plan", "family nlaunch coef_transposes factor_launches factor_pair iterate_transposes small_lds small_opt_in "
                          "ws_alr ws_alr_t ws_aux1 ws_lex cols rows")
Pass = namedtuple("Pass", "kernel lo hi n factor_grid colours chains launches G lds opt_in grid order")
Colour = namedtuple("Colour", "first last grid")


def plan_alr(capi, model, nrows, ncols, nframes=1, it=2, mode=RED_BLACK):
    """The plan of one call under the knobs of the environment; `cols` and `rows` are its two passes."""
    info, rec = (ctypes.c_int * INFO)(), (ctypes.c_int * (2 * PASS))()
    capi.check(capi.load().pdeip_debug_plan_alr(MODEL_ID[model], nrows, ncols, nframes, it, mode, info, rec))
    passes = []
    for d in range(2):
        r = rec[PASS * d:PASS * (d + 1)]
        colours = tuple(Colour(*r[6 + 3 * k:9 + 3 * k]) for k in range(r[5]))
        passes.append(Pass(KERNEL[r[0]], r[1], r[2], r[3], r[4], colours, r[12], r[13], r[14], r[15], bool(r[16]), r[17], (r[18], r[19])))
    return Plan(FAMILY[info[0]], info[1], info[2], info[3], bool(info[4]), info[5], info[6], bool(info[7]), *info[8:12], *passes)
