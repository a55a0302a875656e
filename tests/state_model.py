"""A pure-Python model of what libpdeip.so carries from one exact-order call to the next, and the call sequences of
tests/test_gpu_call_sequences.py.

The one-launch exact-order walkers (k_sor_exact_persist, k_pde8_exact_persist, k_sor_walk) take their (strip, sweep) items from
a schedule table in the per-device scratch slot ws[WS_ORDER].  The table of a call has a shape (B, T, affine): B strips, T
sweeps, XCD-affine lists or one list.  This module follows, through a sequence of events, what that buffer HOLDS and what the
host BELIEVES it holds, under two rule sets:

  "parent"  csrc/pdeip_persist_host.hpp as it was: the host caches the shape of the table it built last and skips
            its table kernel (k_persist_order) on a hit; while the stream is being captured the cache is zeroed, so every captured
            call carries its own table node; a regrown or released buffer drops the cache.  A graph replay rewrites the buffer
            and the host is not told.
  "new"     the host keeps no record: every call builds its table on its stream, in the launch that clears its control block
            (k_persist_setup).

It needs no GPU and does not import the library (a model read off the library would agree with whatever the library does).
tests/test_state_model.py asserts that under the parent's rules every "replay between eager calls" sequence below reaches an
eager walker launch whose buffer is not its own table, and that under the new rules no sequence does.

Events:
  ("eager", call)            an eager exact-order call
  ("capture", name, calls)   the calls enqueued on a capturing stream: nothing runs, the graph `name` gets their nodes
  ("replay", name)           the graph's nodes run
  ("regrow",)                ws[WS_ORDER] is freed and allocated larger (a call that needs more): content undefined
  ("release",)               pdeip_release(): every slot freed
  ("graph", name, calls)     graphs.GraphedRun.__call__: (eager warm-up of the calls + capture, when there is no graph yet or
                             pdeip_workspace_generation() changed) + replay
"""
import math
from collections import namedtuple

NUM_CUS = 256  # MI355X; only decides whether PDEIP_PERSIST_XCD=1 takes the affine lists

# A call: model (device.py entry point and problems.py generator), frame, frames per plane, sweeps
Call = namedtuple("Call", "model nrows ncols nframes it")
Launch = namedtuple("Launch", "event kind want holds")   # a walker launch: index of its event, "eager" | "replay", table it needs / finds


def _ceil(a, b):
    return (a + b - 1) // b


def strips(call, env):
    """B of the call's table: strips of 64 columns; the 5-point models' opt-in walker (PDEIP_EXACT_WALK=1) at PDEIP_WALK_W."""
    w = 64
    if call.model != "pde8" and env.get("PDEIP_EXACT_WALK") == "1" and env.get("PDEIP_WALK_W") in ("32", "48", "64"):
        w = int(env["PDEIP_WALK_W"])
    return _ceil(call.ncols - 2, w)


def shape(call, env):
    """(B, T, affine) of the call's schedule table (persist_prepare)."""
    B, T = strips(call, env), call.it
    affine = 1 if (env.get("PDEIP_PERSIST_XCD", "0") != "0" and call.nframes * T * B <= NUM_CUS) else 0
    return (B, T, affine)


class StaleGraph(Exception):
    """A graph was replayed after the buffers its nodes point into were freed (the callers must re-capture: graphs.py)."""


class Model:
    def __init__(self, rules, env=None):
        assert rules in ("parent", "new")
        self.rules = rules
        self.env = dict(env or {})
        self.buf = None         # shape of the table ws[WS_ORDER] holds (None: undefined content)
        self.cache = None       # parent only: the shape the host believes the buffer holds (None: order_B = order_T = 0)
        self.generation = 0     # pdeip_workspace_generation()
        self.graphs = {}        # name -> (shapes of its walker nodes, generation at capture)
        self.launches = []
        self.captures = 0
        self._event = -1

    # ---- the rules -------------------------------------------------------------------------------------------------------
    def _eager(self, call):
        want = shape(call, self.env)
        if self.rules == "parent":
            if self.cache != want:   # miss: the table kernel on the stream, then the walker
                self.buf = want
                self.cache = want
        else:
            self.buf = want          # every call builds its table
        self.launches.append(Launch(self._event, "eager", want, self.buf))

    def _capture(self, name, calls):
        nodes = []
        for call in calls:
            if self.rules == "parent":
                self.cache = None    # capturing: order_B = order_T = 0 before and after the (captured) build
            nodes.append(shape(call, self.env))   # both rule sets: a node that builds the table (parent: k_persist_order, new: k_persist_setup) in front of the walker node
        self.graphs[name] = (nodes, self.generation)
        self.captures += 1

    def _replay(self, name):
        nodes, generation = self.graphs[name]
        if generation != self.generation:
            raise StaleGraph(name)
        for want in nodes:           # the host is not told: self.cache stays
            self.buf = want
            self.launches.append(Launch(self._event, "replay", want, self.buf))

    def _drop_buffer(self):
        self.buf = None
        self.generation += 1
        if self.rules == "parent":
            self.cache = None        # ws_get / reset_caches: the cached shape goes with its buffer

    # ---- events ------------------------------------------------------------------------------------------------------------
    def apply(self, ev):
        self._event += 1
        kind = ev[0]
        if kind == "eager":
            self._eager(ev[1])
        elif kind == "capture":
            self._capture(ev[1], ev[2])
        elif kind == "replay":
            self._replay(ev[1])
        elif kind in ("regrow", "release"):
            self._drop_buffer()
        elif kind == "graph":
            name, calls = ev[1], ev[2]
            if name not in self.graphs or self.graphs[name][1] != self.generation:
                for call in calls:
                    self._eager(call)
                self._capture(name, calls)
            self._replay(name)
        else:
            raise ValueError(ev)

    def run(self, events):
        for ev in events:
            self.apply(ev)
        return self

    def wrong_tables(self, kind=None):
        """The walker launches that found another table than their own."""
        return [l for l in self.launches if l.holds != l.want and (kind is None or l.kind == kind)]


# ---- the sequences of tests/test_gpu_call_sequences.py -------------------------------------------------------------------
# C.1, replay between eager calls.  X: the eager call; Y: the calls inside the graph (the last one's table is what a replay leaves
# in the buffer).  Frames are small; with the default strips B = ceil((ncols - 2) / 64).
Sequence = namedtuple("Sequence", "name env X Y")

REPLAY_SEQUENCES = [
    # as many items, another B: (3, 4) against (4, 3)
    Sequence("equal_items", {}, Call("elin4", 40, 150, 1, 4), (Call("elin4", 33, 230, 1, 3),)),
    # Y larger: (2, 2) against (5, 4) x 2 frames, the 9-point walker on both sides
    Sequence("graph_larger", {}, Call("pde8", 37, 100, 1, 2), (Call("pde8", 50, 300, 2, 4),)),
    # Y smaller: (6, 3) against (1, 2) x 3 frames, single-field models
    Sequence("graph_smaller", {}, Call("disp4", 45, 330, 1, 3), (Call("pde4", 30, 60, 3, 2),)),
    # two calls in the graph, the 9-point one first: the buffer keeps the LAST one's table, (2, 6) against X's (3, 4)
    Sequence("two_calls", {}, Call("elin4", 40, 150, 1, 4), (Call("pde8", 41, 200, 1, 3), Call("elin4", 35, 100, 1, 6))),
    # the opt-in walker at 48 columns per strip: (4, 4) against (5, 3)
    Sequence("walk48", {"PDEIP_EXACT_WALK": "1", "PDEIP_WALK_W": "48"}, Call("elin4", 40, 150, 1, 4), (Call("elin4", 33, 230, 1, 3),)),
    # the XCD-affine lists: (3, 4, affine) against (4, 3, affine)
    Sequence("xcd", {"PDEIP_PERSIST_XCD": "1"}, Call("elin4", 40, 150, 1, 4), (Call("elin4", 33, 230, 1, 3),)),
]
REPLAYS = 2   # eager(X), replay(Y), eager(X), replay(Y), and X once more


def replay_events(seq):
    """Every shape warmed up (X eagerly; Y by the GraphedRun's own first call: warm-up, capture, replay), then
    eager(X), replay(Y) REPLAYS times, then eager(X)."""
    ev = [("eager", seq.X), ("graph", seq.name, seq.Y)]
    for _ in range(REPLAYS):
        ev += [("eager", seq.X), ("graph", seq.name, seq.Y)]
    return ev + [("eager", seq.X)]


# C.2, a GraphedRun used again after the generation changed: the next use re-captures.  BIG needs a larger WS_ORDER (and every
# other slot) than anything before it.
REGROW = Sequence("regrow", {}, Call("elin4", 40, 150, 1, 4), (Call("elin4", 33, 230, 1, 3), Call("pde8", 41, 200, 1, 3)))
REGROW_BIG = Call("elin4", 300, 1400, 1, 9)


def regrow_events(seq=REGROW, big=REGROW_BIG):
    g = ("graph", seq.name, seq.Y)
    return [("eager", seq.X), g, g, ("regrow",), ("eager", big), g, ("eager", seq.X), g, ("release",), ("eager", seq.X), g, ("eager", seq.X), g, ("eager", seq.X)]


# D, the driver-level form in tests/test_gpu_drivers.py::test_graph_replay_gives_the_eager_bits: the late-linearisation driver relaxes
# every scale of its pyramid (coarsest first) firstLoop x secondLoop times with ONE sweep count, param.iter.  A frame of at most 66
# columns is one strip on every scale, so the first walker launch of an eager run has the table shape of its last; the replayed
# graph of the full frame leaves the table of its finest scale behind.
DRIVER_FULL, DRIVER_SMALL = (252, 316), (60, 64)   # the Yosemite frames and the crop the test runs eagerly
DRIVER_ITER, DRIVER_LOOPS = 4, 4 * 4                # drivers.ND_DEFAULTS: iter, firstLoop x secondLoop


def driver_calls(frame, scl_factor=0.75, min_size=20):
    """The exact-order solver calls of one driver run, in order (pyramid.build_dev: scales shrink by ceil(0.75 n) until one side
    is at most 20; the run goes from the coarsest scale to the finest)."""
    shapes = [frame]
    while True:
        nr, nc = int(math.ceil(shapes[-1][0] * scl_factor)), int(math.ceil(shapes[-1][1] * scl_factor))
        shapes.append((nr, nc))
        if nr <= min_size or nc <= min_size:
            break
    return tuple(Call("llin4", nr, nc, 1, DRIVER_ITER) for nr, nc in reversed(shapes) for _ in range(DRIVER_LOOPS))


def driver_events():
    """An eager run of the small frame, then twice: the graphed run of the full frame and the small frame eagerly again."""
    full, small = driver_calls(DRIVER_FULL), driver_calls(DRIVER_SMALL)
    ev = [("eager", c) for c in small]
    for _ in range(2):
        ev += [("graph", "driver", full)] + [("eager", c) for c in small]
    return ev


def items(call, env):
    B, T, _ = shape(call, env)
    return B * T
