"""CPU side of the seam tests: the model of the launch logic (tests/seam_model.py) against the figures the sources state, and
the proof that the case lists which tests/test_gpu_seams.py runs reach every seam -- counting a case only towards the kernels
its launch chain really runs."""
from seam_model import (
    CASES, CLASS, alr_cases, alr_launches, alr_small_lds_bytes, case_id, chain, coverage_gaps, family_of, geometry,
    kernels_of, rbp_fits, rbp_lead, rbp_waves_per_sweep, small_launches,
)


# ---- the model against the figures the sources state ----------------------------------------------------------------------
def test_model_restates_the_launch_logic():
    assert all(rbp_fits(m) for m in ("elin4", "llin4", "disp4", "dispsym4", "pde4")) and not rbp_fits("pde8")
    assert [rbp_waves_per_sweep(m) for m in ("elin4", "llin4", "disp4", "pde4")] == [2, 2, 1, 1]
    assert rbp_lead("elin4") == 5  # "lets the lead grow from four to five for the coupled models" (pdeip_sor_rbp.hpp)
    # iter = 8: two pipelined launches against four of k_sor_rb; 9 = 4 + 4 + 1; 7 = 4 + 2 + 1
    assert chain("rbp", 8) == [4, 4] and chain("rb", 8) == [2, 2, 2, 2] and chain("rbp", 9) == [4, 4, 1] and chain("rbp", 7) == [4, 2, 1]
    assert chain("rb", 5) == [2, 2, 1] and chain("pde8", 3) == [2, 1] and chain("rbp", 3) == [2, 1]
    # which kernels a chain runs: fewer than four sweeps never reach the pipeline, an even count never the one-sweep kernels
    assert kernels_of("rbp", 8) == ["k_sor_rbp"] and kernels_of("rbp", 7) == ["k_sor_rbp"] and kernels_of("rb", 1) == ["k_sor_rb one-sweep"]
    assert kernels_of("rb", 4) == ["k_sor_rb two-sweep"] and kernels_of("pde8", 3) == ["k_pde8_colour2", "k_pde8_colour"]
    assert family_of("elin4", 244, 26, it=3, small=False) == "rb" and family_of("disp4", 1024, 2048, it=2, small=False) == "rb"
    assert geometry("k_pde8_colour", "pde8", 249, 5, 2).row_tiles == 1 and geometry("k_pde8_colour", "pde8", 252, 5, 2).last_tile_rows == 4
    g = geometry("rbp", "elin4", 2160, 3840, 138)
    assert (g.row_tiles, g.last_tile_rows, g.strips, g.last_strip, g.vec, g.last_in_halo) == (9, 240, 28, 114, True, False)
    g = geometry("rb", "elin4", 249, 38, 13)
    assert (g.row_tiles, g.last_tile_rows, g.strips, g.last_strip, g.vec, g.grid) == (1, 249, 3, 12, False, 1)
    assert geometry("rbp", "elin4", 4, 9, 8).last_in_halo and geometry("pde8", "pde8", 241, 5, 2).row_tiles == 1
    assert geometry("pde8", "pde8", 242, 5, 2).row_tiles == 2 and geometry("rb", "disp4", 497, 5, 2).row_tiles == 2
    # the pipeline takes a single-field model from 2^21 pixels on, and only whole lanes of four rows behind aligned planes
    assert family_of("disp4", 1024, 2048, small=False) == "rbp" and family_of("disp4", 1024, 2047, small=False) == "rb"
    assert family_of("elin4", 33, 29, small=False) == "rb" and family_of("elin4", 68, 120, small=False) == "rbp"
    assert family_of("elin4", 68, 120, small=False, aligned=False) == "rb" and family_of("elin4", 68, 120, small=False, pipe=False) == "rb"
    # k_sor_small: the whole call in one launch; a frame that has to be cut runs four sweeps per launch (9 = 4 + 4 + 1)
    assert small_launches("elin4", 24, 40, 1, 9) == 1 and small_launches("elin4", 135, 240, 1, 9) == 3 and small_launches("elin4", 135, 240, 1, 4) == 1
    assert small_launches("elin4", 1080, 1920, 1, 4) is None
    # k_alr_small: up to 6144 pixels, the whole call in one launch
    assert alr_small_lds_bytes(64, 96, False) == 48 * 65 * 20 <= 150 * 1024
    assert alr_launches("elin4", 64, 96, 3) == 1 and alr_launches("elin4", 64, 97, 3) == 1 + 2 + 3 * 6
    assert alr_launches("elin4", 64, 96, 3, small=False, pair=False) == 1 + 2 + 3 * 10
    assert alr_launches("pde8", 3, 3, 5, small=False) == 1 + 2 + 1 * 4 and alr_launches("disp4", 3, 40, 1, small=False) == 1 + 2 + 6


def test_cases_cover_every_seam():
    assert coverage_gaps() == []


def test_every_case_class_is_needed():
    """Dropping any one class of cases leaves a hole that the coverage test names."""
    for group in ("A", "An", "B", "C", "D"):
        assert coverage_gaps(cases=[c for c in CASES if c.group != group]), group
    for cls in ("coupled", "single", "pde8"):
        assert coverage_gaps(cases=[c for c in CASES if CLASS[c.model] != cls]), cls
    assert coverage_gaps(alr=[c for c in alr_cases() if c.small])
    assert coverage_gaps(alr=[c for c in alr_cases() if not c.small])
    assert coverage_gaps(alr=[c for c in alr_cases() if c.pair])
    assert len({case_id(c) for c in CASES}) == len(CASES)
    # a case labelled with the pipeline that is too short to launch it is named, not credited
    short = CASES[0]._replace(it=3)
    assert any("never launch k_sor_rbp" in g for g in coverage_gaps(cases=CASES + [short]))
    # and a case counts only towards the kernels it runs: with every pipeline case cut to three sweeps the pipeline's sets are empty
    assert any(g.startswith("k_sor_rbp/coupled last-strip width") for g in coverage_gaps(cases=[c._replace(it=3, family="rb") if c.family == "rbp" else c for c in CASES]))
