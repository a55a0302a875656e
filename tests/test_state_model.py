"""CPU side of the call-sequence tests: the model of the state the library carries between exact-order calls
(tests/state_model.py), the proof that every "replay between eager calls" sequence which tests/test_gpu_call_sequences.py runs
is a witness of the stale schedule table under the parent's rules -- the mutation evidence for those tests -- and that no
sequence is one under the new rules."""
import pytest

from state_model import (DRIVER_FULL, DRIVER_SMALL, REGROW, REGROW_BIG, REPLAY_SEQUENCES, Call, Model, StaleGraph, items, driver_calls, driver_events, regrow_events,
                         replay_events, shape, strips)


def test_model_restates_the_table_shapes():
    assert strips(Call("elin4", 34, 60, 1, 4), {}) == 1 and strips(Call("elin4", 270, 480, 1, 4), {}) == 8
    assert strips(Call("elin4", 2160, 3840, 1, 4), {}) == 60 and strips(Call("pde8", 90, 330, 2, 3), {}) == 6
    walk = {"PDEIP_EXACT_WALK": "1", "PDEIP_WALK_W": "32"}
    assert strips(Call("elin4", 40, 150, 1, 4), walk) == 5 and strips(Call("pde8", 40, 150, 1, 4), walk) == 3   # the 9-point walker has one width
    assert strips(Call("elin4", 40, 150, 1, 4), {"PDEIP_WALK_W": "32"}) == 3                                      # not without the opt-in
    xcd = {"PDEIP_PERSIST_XCD": "1"}
    assert shape(Call("elin4", 40, 150, 1, 4), xcd) == (3, 4, 1) and shape(Call("elin4", 40, 150, 1, 4), {}) == (3, 4, 0)
    assert shape(Call("elin4", 150, 330, 2, 40), xcd) == (6, 40, 0)   # more workgroups than compute units: one list whatever the knob


def test_the_failing_sequence_of_the_issue():
    """Warm up and capture a graph whose last call has shape Y; eager X; replay; eager X again: it hits the cache and walks Y's."""
    X, Y = Call("elin4", 40, 150, 1, 4), Call("elin4", 33, 230, 1, 3)
    ev = [("eager", Y), ("capture", "g", (Y,)), ("eager", X), ("replay", "g"), ("eager", X)]
    m = Model("parent").run(ev)
    assert [(l.event, l.kind, l.want, l.holds) for l in m.wrong_tables()] == [(4, "eager", (3, 4, 0), (4, 3, 0))]
    assert Model("new").run(ev).wrong_tables() == []
    # without the replay the parent's cache is right, and the capture-time direction was handled: a graph captured while the cache
    # says Y still builds its own table on replay
    assert Model("parent").run([("eager", Y), ("capture", "g", (Y,)), ("eager", X), ("eager", X)]).wrong_tables() == []
    assert Model("parent").run([("eager", Y), ("capture", "g", (Y,)), ("eager", X), ("replay", "g"), ("replay", "g")]).wrong_tables() == []


@pytest.mark.parametrize("seq", REPLAY_SEQUENCES, ids=lambda s: s.name)
def test_every_replay_sequence_is_a_witness_under_the_parents_rules(seq):
    m = Model("parent", seq.env).run(replay_events(seq))
    bad = m.wrong_tables()
    assert bad, seq.name
    want_x, left_by_y = shape(seq.X, seq.env), shape(seq.Y[-1], seq.env)
    for l in bad:   # always the eager call, walking what the graph's last call left behind
        assert (l.kind, l.want, l.holds) == ("eager", want_x, left_by_y), l
    assert m.captures == 1   # nothing regrows mid-sequence: one capture, then replays
    assert Model("parent", seq.env).run(replay_events(seq)).wrong_tables("replay") == []


@pytest.mark.parametrize("seq", REPLAY_SEQUENCES + [REGROW], ids=lambda s: s.name)
def test_no_sequence_walks_a_wrong_table_under_the_new_rules(seq):
    ev = regrow_events() if seq is REGROW else replay_events(seq)
    m = Model("new", seq.env).run(ev)
    assert m.launches and m.wrong_tables() == []


def test_replay_sequences_cover_every_size_relation():
    """Y's item count against X's: equal with another B, larger, smaller; both walkers and a single-field model on the eager side;
    a graph of two calls; one sequence through the opt-in walker at a width of its own, one with the XCD-affine lists."""
    rel = set()
    for s in REPLAY_SEQUENCES:
        x, y = items(s.X, s.env), items(s.Y[-1], s.env)
        assert shape(s.X, s.env) != shape(s.Y[-1], s.env), s.name
        rel.add("equal" if x == y and strips(s.X, s.env) != strips(s.Y[-1], s.env) else ("larger" if y > x else ("smaller" if y < x else "same")))
    assert rel == {"equal", "larger", "smaller"}
    x0, y0 = REPLAY_SEQUENCES[0].X, REPLAY_SEQUENCES[0].Y[-1]
    assert (shape(x0, {})[:2], shape(y0, {})[:2]) == ((3, 4), (4, 3))
    assert {s.X.model for s in REPLAY_SEQUENCES} >= {"elin4", "pde8", "disp4"}
    assert {c.model for s in REPLAY_SEQUENCES for c in s.Y} >= {"elin4", "pde8", "pde4"}
    assert any(len(s.Y) == 2 for s in REPLAY_SEQUENCES)
    assert any(s.env.get("PDEIP_EXACT_WALK") == "1" and s.env.get("PDEIP_WALK_W") in ("32", "48") for s in REPLAY_SEQUENCES)
    assert any(shape(s.X, s.env)[2] == 1 and shape(s.Y[-1], s.env)[2] == 1 for s in REPLAY_SEQUENCES)
    assert len({s.name for s in REPLAY_SEQUENCES}) == len(REPLAY_SEQUENCES)


def test_regrow_and_release_force_a_new_capture():
    """The generation changes with a regrown or released buffer: a GraphedRun re-captures (three captures in the sequence), and
    replaying the old graph instead would run nodes that point into freed buffers."""
    for rules in ("parent", "new"):
        m = Model(rules).run(regrow_events())
        assert m.captures == 3 and m.generation == 2
    assert items(REGROW_BIG, {}) > max(items(c, {}) for c in (REGROW.X,) + REGROW.Y)
    m = Model("new").run([("graph", "g", REGROW.Y), ("regrow",)])
    with pytest.raises(StaleGraph):
        m.apply(("replay", "g"))


def test_the_driver_level_sequence_is_a_witness_too():
    """tests/test_gpu_drivers.py runs the small frame eagerly between two uses of the full frame's graph: every scale of the small
    frame has the table (1, iter), the graph leaves the full frame's finest table, five strips; under the parent's rules the first
    walker launch of the eager run after a replay walks that one."""
    small, full = driver_calls(DRIVER_SMALL), driver_calls(DRIVER_FULL)
    assert {shape(c, {}) for c in small} == {(1, 4, 0)} and shape(full[-1], {}) == (5, 4, 0)
    assert (small[-1].nrows, small[-1].ncols) == DRIVER_SMALL and (full[-1].nrows, full[-1].ncols) == DRIVER_FULL
    assert min(small[0].nrows, small[0].ncols) <= 20 < min(small[16].nrows, small[16].ncols)
    bad = Model("parent").run(driver_events()).wrong_tables()
    assert bad and all((l.kind, l.want, l.holds) == ("eager", (1, 4, 0), (5, 4, 0)) for l in bad)
    assert Model("new").run(driver_events()).wrong_tables() == []
