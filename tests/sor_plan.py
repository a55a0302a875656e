"""What the seam tests share: the knobs() context, the knobs a point-SOR case sets, and a reader of pdeip_debug_plan_sor (the
library's own launch plan: csrc/pdeip_sor_plan.hpp), which needs no GPU when the three device facts are passed."""
import contextlib
import ctypes
import os
from collections import namedtuple

KNOBS = ("PDEIP_RB_SMALL", "PDEIP_RB_PIPE", "PDEIP_RBP_TJ", "PDEIP_RB_TJ", "PDEIP_RBP_SERPENTINE", "PDEIP_ALR_SMALL", "PDEIP_ALR_PAIR",
         "PDEIP_ALR_SCAN", "PDEIP_EXACT_PERSIST", "PDEIP_EXACT_WALK", "PDEIP_PDE8_PERSIST")  # the last three: the exact-order forms (test_gpu_range.py)


@contextlib.contextmanager
def knobs(**kv):
    """Set the given knobs (None: unset), clear the others, and put everything back."""
    old = {k: os.environ.get(k) for k in KNOBS}
    try:
        for k in KNOBS:
            v = kv.get(k)
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def point_case_knobs(c):
    """The knobs that force a seam_model.Case onto its family and strip width."""
    return dict(PDEIP_RB_SMALL=1 if c.small else 0, PDEIP_RB_PIPE=0 if c.group == "C" else 1, PDEIP_RBP_SERPENTINE=c.serp,
                PDEIP_RBP_TJ=c.tj if c.family == "rbp" else None, PDEIP_RB_TJ=c.tj if c.group == "C" else None)


MODEL_ID = {"elin4": 0, "llin4": 1, "disp4": 2, "pde4": 3, "pde8": 4, "dispsym4": 5}  # PDEIP_PLAN_* of include/pdeip.h
FAMILY = {0: None, 1: "exact", 2: "small", 3: "rb", 4: "rbp", 5: "pde8"}
FORM = {0: None, 1: "persist", 2: "walk", 3: "front"}
KERNEL = {1: "k_sor_rbp", 2: "k_sor_rb two-sweep", 3: "k_sor_rb one-sweep", 4: "k_sor_small", 5: "k_pde8_colour2", 6: "k_pde8_colour",
          7: "pack", 8: "persist", 9: "walk", 10: "derive", 11: "front", 12: "borders"}
CALLER, SCRATCH, DST = 0, 1, 2
Plan = namedtuple("Plan", "family form closing_copy opening_copy persist_setup A B NC W last_m launches")
Launch = namedtuple("Launch", "kernel sweeps first tj tiles units grid src dst")


def plan_sor(capi, model, nrows, ncols, nframes=1, it=4, mode=1, aligned=True, has_dst=False, cus=256, rb2_slots=8192, rbp_slots=256):
    """The plan of one call under the knobs of the environment.  Device facts of 0 are asked from the current device."""
    lib = capi.load()
    info = (ctypes.c_int * 11)()
    head = (MODEL_ID[model], nrows, ncols, nframes, it, mode, int(aligned), int(has_dst), cus, rb2_slots, rbp_slots, info)
    capi.check(lib.pdeip_debug_plan_sor(*head, None, 0))
    rec = (ctypes.c_int * (9 * max(1, info[10])))()
    capi.check(lib.pdeip_debug_plan_sor(*head, rec, info[10]))
    launches = [Launch(KERNEL[rec[9 * i]], *rec[9 * i + 1:9 * i + 9]) for i in range(info[10])]
    return Plan(FAMILY[info[0]], FORM[info[1]], bool(info[2]), bool(info[3]), bool(info[4]), *info[5:10], launches)
