"""GPU tests of the generic accumulation's work list (csrc/mfd_worklist.hpp: k_wl_stack, k_wl_buffer) on dependency graphs handed
to it directly as proportion rasters, so that the paths a fractal DEM does not reach are PROVEN to run:

  * the spill of k_wl_stack (a wavefront's LDS stack of WL_CAP = 1536 cells is full: by-products go to the next launch),
  * the hand-over of k_wl_buffer (a thread's LDS buffer of WL_BUF = 20 cannot take 8 more: the current cell goes to the
    next launch unprocessed),
  * the pop of idle lanes (min(popcount(idle), sp) entries, ranked by mbcnt), eight donors completing one cell at the same
    moment, pushes of several cells by one lane, cells on the raster's edge, NoData receivers, a cycle,
  * the compact D-infinity accessor (DinfAcc) against the nine-float one (PropsAcc) on the same proportions,
  * the device entries rdgpu_flow_accumulation_dev_f64 and rdgpu_fa_mfd_dev_* on the caller's stream.

Which path ran is read from the launch count (rd.flow_accumulation_rounds()); the bounds asserted on it follow from WL_CAP
and WL_BUF (see EXPECT_ROUNDS), not from a measurement.  All graphs carry shares of 1.0 and are forests (hubs: sums of nine
integers), so every value is a small integer, the order of summation cannot matter and the comparison is exact.

Proportions layout [h, w, 9]: slot 0 is the marker (-2 NoData, 0 has flow, -1 no flow), slots 1..8 the shares (-1 none) to
the neighbours 1 left, 2 up-left, 3 up, 4 up-right, 5 right, 6 down-right, 7 down, 8 down-left.  Every cell that a builder
does not name is NoData, so the first work list is exactly the graph's sources in row-major order: that decides which lane
of which wavefront holds which cell.  Cells on the raster's edge never get a positive share (the FM_* functions never give
them one; the reference's queue would forward such a share while the engine stops at the edge)."""
import numpy as np
import pytest

from richdem_amd.synth import fractal_dem

pytestmark = pytest.mark.gpu

DX = (0, -1, -1, 0, 1, 1, 1, 0, -1)
DY = (0, 0, -1, -1, -1, 0, 1, 1, 1)
LEFT, UP, RIGHT, DOWN = 1, 3, 5, 7

STACK_BELOW = [None, "0", "4000000000"]      # the default; always k_wl_buffer; always k_wl_stack
MODE = {None: "default", "0": "round", "4000000000": "stack"}


def ulp_diff_f32(a, b):
    a = np.ascontiguousarray(a, np.float32)
    b = np.ascontiguousarray(b, np.float32)
    ia = a.view(np.int32).astype(np.int64)
    ib = b.view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia)
    ib = np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    return np.abs(ia - ib)


# ---- proportion rasters -----------------------------------------------------------------------------------
def blank(h, w):
    p = np.full((h, w, 9), -1.0, np.float32)
    p[..., 0] = -2.0
    return p


def put(p, y, x, *ns, marker=None):
    """name cell (y, x): a data cell that gives share 1 to each neighbour in ns"""
    p[y, x, 0] = (0.0 if ns else -1.0) if marker is None else marker
    for n in ns:
        p[y, x, n] = 1.0


def chain(p, y, x, n, length):
    """`length` cells from (y, x) on in direction n, each giving share 1 to the next; the last one gives nothing"""
    for k in range(length):
        put(p, y + k * DY[n], x + k * DX[n], *((n,) if k < length - 1 else ()))


def check_raster(p):
    edge = np.ones(p.shape[:2], bool)
    edge[1:-1, 1:-1] = False
    assert not (p[edge][:, 1:] > 0).any(), "a cell on the raster's edge has a positive share"
    return p


def comb(lengths, side=3, pitch=4, to_edges=False, nodata_heads=False):
    """Horizontal trunks, `pitch` rows apart; trunk cell (y, x) feeds the next trunk cell (right) and the head of a side
    chain of `side` cells running down.  The engine continues inline with the lowest n: a lane walks its trunk and
    pushes one side head per step (the trunk's last cell has the side chain as its only receiver: no push)."""
    nt, width = len(lengths), max(lengths) + 2
    p = blank(nt * pitch + 2, width)
    h = p.shape[0]
    for i, ln in enumerate(lengths):
        y = 1 + i * pitch
        for x in range(1, ln + 1):
            put(p, y, x, *((RIGHT, DOWN) if x < ln else (DOWN,)))
            if nodata_heads and (i + x) % 5 == 0:
                continue          # this side chain stays NoData (all of it, so that the trunk heads stay the only sources)
            chain(p, y + 1, x, DOWN, side + 1 if to_edges and i == nt - 1 else side)
        if to_edges:              # the trunk runs on into the last column: an edge cell that receives and passes nothing
            p[y, ln, RIGHT] = 1.0
            put(p, y, ln + 1, marker=0.0)
    if to_edges:
        assert width == lengths[0] + 2 and (p[h - 1, 1:-1, 0] == -1.0).all()
        p[h - 1, 1:-1, 0] = 0.0   # the last trunk's side chains end in the bottom row
    return check_raster(p)


def comb_ns(ntrunks=64, length=40, side=3):
    """Each trunk cell feeds up, right and down: the lane continues into the UP chain (lowest n) and pushes the trunk
    itself and the down head, two pushes per step."""
    pitch = 2 * side + 1
    p = blank(ntrunks * pitch + 2, length + 2)
    for i in range(ntrunks):
        y = 1 + side + i * pitch
        for x in range(1, length + 1):
            put(p, y, x, *((UP, RIGHT, DOWN) if x < length else (UP, DOWN)))
            chain(p, y - 1, x, UP, side)
            chain(p, y + 1, x, DOWN, side)
    return check_raster(p)


def hubs(size=150):
    """A 3-pitch lattice of hubs; each hub has no shares, its eight neighbours are sources that feed it: eight threads
    complete one cell at the same moment, exactly one of them sees the counter reach zero."""
    p = blank(size, size)
    centres = range(2, size - 2, 3)
    for y in centres:
        for x in centres:
            put(p, y, x)
            for n in range(1, 9):
                put(p, y + DY[n], x + DX[n], n + 4 if n <= 4 else n - 4)
    return check_raster(p), [(y, x) for y in centres for x in centres]


def stars(k=8, pitch=7):
    """A lattice of sources that feed all eight neighbours, each the head of a straight outward ray of 2 more cells: one
    lane pushes 7 cells at once (the per-lane prefix with no > 1; nb = 7 after one step of k_wl_buffer)."""
    p = blank(k * pitch + 2, k * pitch + 2)
    for j in range(k):
        for i in range(k):
            y, x = 4 + j * pitch, 4 + i * pitch
            put(p, y, x, *range(1, 9))
            for n in range(1, 9):
                chain(p, y + DY[n], x + DX[n], n, 3)
    return check_raster(p)


def cycle():
    """A chain of 10 cells feeds a 2 x 2 ring whose cells pass share 1 round the ring: the ring's counters never reach
    zero, the ring keeps its weights plus what the chain delivered."""
    p = blank(6, 15)
    for x in range(1, 11):
        put(p, 2, x, RIGHT)
    put(p, 2, 11, RIGHT)
    put(p, 2, 12, DOWN)
    put(p, 3, 12, LEFT)
    put(p, 3, 11, UP)
    return check_raster(p)


RASTERS = {
    "comb_spill": lambda: comb([40] * 64),                                   # 258 x 42: steps 25-39 of one wavefront spill
    "comb_control": lambda: comb([40] * 8),                                  # 34 x 42: 56 idle lanes pop, nothing spills
    "comb_two_waves": lambda: comb([40] * 128),                              # two wavefronts of one block, a stack each
    "comb_ragged": lambda: comb([20 + (7 * i) % 61 for i in range(64)]),     # lanes go idle at different steps
    "comb_short": lambda: comb([12] * 64),                                   # 11 pushes per thread fit in WL_BUF
    "comb_ns": comb_ns,
    "comb_to_edges": lambda: comb([40] * 64, to_edges=True),
    "comb_nodata": lambda: comb([40] * 64, nodata_heads=True),
    "hubs": lambda: hubs()[0],
    "stars": stars,
    "cycle": cycle,
}

# Launch counts that follow from WL_CAP = 1536 and WL_BUF = 20 (op, bound), by (raster, forced schedule):
#  stack, 64 trunks of 40: every step of the wavefront pushes 64 side heads (51 or 52 in comb_nodata, 39 steps: > 1536 in
#    all) and no lane is idle before the trunks end, so the stack is full after 24 steps and the later steps spill: a
#    second launch.  8 trunks: 56 idle lanes pop what 8 push; 64 trunks of 12: 64 x 11 = 704 entries: one launch.
#  round, trunks of 12: a thread buffers 11 side heads (nb + 8 <= 20 throughout), the heads are round two and each walks
#    its 3-cell chain inline.  Trunks of 40: after 13 buffered heads (nb + 8 > 20) the thread hands its trunk cell over, so
#    the trunk alone takes three launches and its last side heads a fourth.
EXPECT_ROUNDS = {
    ("comb_control", "stack"): ("==", 1), ("comb_short", "stack"): ("==", 1),
    ("comb_spill", "stack"): (">=", 2), ("comb_two_waves", "stack"): (">=", 2),
    ("comb_to_edges", "stack"): (">=", 2), ("comb_nodata", "stack"): (">=", 2),
    ("comb_short", "round"): ("==", 2), ("comb_spill", "round"): (">=", 3),
    # the chain is one thread's inline walk and the ring never completes: "a handful" of launches at the most
    ("cycle", "stack"): ("<=", 4), ("cycle", "round"): ("<=", 4), ("cycle", "default"): ("<=", 4),
}


def check_rounds(name, mode, rounds):
    op, bound = EXPECT_ROUNDS.get((name, mode), (">=", 1))
    ok = {"==": rounds == bound, ">=": rounds >= bound, "<=": rounds <= bound}[op]
    assert ok, f"{name} under {mode}: {rounds} launches, expected {op} {bound}"


def assert_exact_integers(exp, name):
    data = exp[exp != -1.0]
    assert np.array_equal(data, np.rint(data)) and (np.abs(data) < 2.0 ** 53).all(), name


@pytest.fixture(scope="module")
def graphs(orc):
    """name -> (props, weights, the oracle's accumulation with unit weights, ... with the weights); computed once"""
    out = {}
    for k, (name, mk) in enumerate(RASTERS.items()):
        p = mk()
        w = np.random.default_rng(100 + k).integers(1, 8, p.shape[:2]).astype(np.float64)
        e1, ew = orc.port.flow_accumulation(p), orc.port.flow_accumulation(p, w)
        assert_exact_integers(e1, name)
        assert_exact_integers(ew, name)
        for a in (p, w, e1, ew):
            a.setflags(write=False)
        out[name] = (p, w, e1, ew)
    return out


# ---- 1, 2: the work list on hand-made graphs --------------------------------------------------------------
@pytest.mark.parametrize("stack_below", STACK_BELOW, ids=lambda s: MODE[s])
@pytest.mark.parametrize("name", list(RASTERS))
def test_worklist_graph_vs_oracle(rd, graphs, monkeypatch, name, stack_below):
    if stack_below is not None:
        monkeypatch.setenv("RDGPU_MFD_STACK_BELOW", stack_below)
    else:
        monkeypatch.delenv("RDGPU_MFD_STACK_BELOW", raising=False)
    p, w, e1, ew = graphs[name]
    for weights, exp in ((None, e1), (w, ew)):
        got = rd.FlowAccumFromProps(p) if weights is None else rd.FlowAccumFromProps(p, weights)
        rounds = rd.flow_accumulation_rounds()
        print(f"rounds {name} {MODE[stack_below]} {'unit' if weights is None else 'weighted'}: {rounds}")
        bad = got != exp
        assert not bad.any(), (name, MODE[stack_below], int(bad.sum()), np.argwhere(bad)[:4].tolist())
        check_rounds(name, MODE[stack_below], rounds)


def test_graphs_are_what_the_cases_need(graphs):
    """The rasters themselves (no engine): sources, sizes and the values that the descriptions above promise."""
    def sources(p):
        h, w, _ = p.shape
        donors = np.zeros((h, w), int)
        for n in range(1, 9):
            ys, xs = np.nonzero(p[..., n] > 0)
            np.add.at(donors, (ys + DY[n], xs + DX[n]), 1)
        return (donors == 0) & (p[..., 0] != -2.0)

    for name, ntr in (("comb_spill", 64), ("comb_control", 8), ("comb_two_waves", 128), ("comb_ragged", 64), ("comb_short", 64),
                      ("comb_ns", 64), ("comb_to_edges", 64), ("comb_nodata", 64)):
        s = sources(graphs[name][0])
        assert s.sum() == ntr and s[:, 1].sum() == ntr, name              # the trunk heads and nothing else
    assert graphs["comb_spill"][0].shape == (258, 42, 9) and graphs["comb_control"][0].shape == (34, 42, 9)
    p, _, e1, _ = graphs["comb_to_edges"]
    assert (p[1:-1:4, -1, 0] == 0.0).all() and (e1[1:-1:4, -1] == 41.0).all()      # the trunks' ends in the last column
    assert (p[-1, 1:-1, 0] == 0.0).all() and (e1[-1, 1:-1] == np.arange(1, 41) + 4).all()   # the chains' ends in the bottom row
    p, _, e1, _ = graphs["comb_nodata"]
    heads = p[2::4, 1:41, 0]                                                         # the side heads, trunk by trunk
    assert (heads == -2.0).sum() == 64 * 8 and (e1[2::4, 1:41][heads == -2.0] == -1.0).all()
    p, w, e1, ew = graphs["hubs"]
    centres = hubs()[1]
    assert len(centres) == 49 * 49
    for y, x in centres[::97]:
        assert e1[y, x] == 9.0 and ew[y, x] == w[y - 1:y + 2, x - 1:x + 2].sum()
    assert sources(graphs["stars"][0]).sum() == 64
    p, w, e1, ew = graphs["cycle"]
    assert e1[2, 11] == 11.0 and e1[2, 12] == 1.0 and e1[3, 12] == 1.0 and e1[3, 11] == 1.0
    assert ew[2, 11] == w[2, 1:12].sum()


def test_edge_cells_pass_nothing_on(rd, orc, graphs, monkeypatch):
    """The engine's own contract for a proportions array that no FM_* function produces: a cell on the raster's edge with a
    positive share is not a donor (k_mfd_init counts interior donors only) and passes nothing on (both kernels stop at
    the edge).  comb_to_edges with shares put on its edge cells -- the trunks' ends point back into their trunks, the
    bottom row points up into the side chains -- must therefore give what the oracle gives WITHOUT those shares.  (With
    them the oracle's queue forwards the flow: another contract, not compared.)"""
    p, w, e1, ew = graphs["comb_to_edges"]
    q = p.copy()
    q[1:-1:4, -1, LEFT] = 1.0
    q[-1, 1:-1, UP] = 1.0
    for sb in STACK_BELOW:
        if sb is not None:
            monkeypatch.setenv("RDGPU_MFD_STACK_BELOW", sb)
        assert np.array_equal(rd.FlowAccumFromProps(q), e1), MODE[sb]
        assert np.array_equal(rd.FlowAccumFromProps(q, w), ew), MODE[sb]


# ---- 3: the compact D-infinity accessor through the same kernels ------------------------------------------
EXACT = [(1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (1, -1), (-1, 1), (-1, -1)]              # one receiver per cell
BETWEEN = [(1, 3), (1, -3), (-1, 3), (-1, -3), (3, 1), (3, -1), (-3, 1), (-3, -1)]          # two receivers per cell
ND = np.int32(-9999)


def plane(a, b, hole=False):
    y, x = np.mgrid[0:96, 0:130]
    z = (a * x + b * y + 1000).astype(np.int32)
    if hole:
        z[40:52, 55:75] = ND
    return z


PLANES = [(f"{a:+d}{b:+d}", a, b, False) for a, b in EXACT + BETWEEN] + [("-3+1_hole", -3, 1, True)]


@pytest.fixture(scope="module")
def planes(rd, orc):
    """name -> (z, the engine's proportions, the oracle's accumulation of THOSE proportions): the trigonometry stays out of
    the accumulation's comparison (a one-ULP difference in a plane's one repeated proportion would compound over 130
    generations)"""
    out = {}
    for name, a, b, hole in PLANES:
        z = plane(a, b, hole)
        props = rd.FlowProportions(z, "Dinf", nodata=ND)
        out[name] = (z, props, orc.port.flow_accumulation(props))
    return out


def test_plane_proportions(orc, planes):
    """FM_Tarboton on the 17 planes against the oracle, as test_mfd_gpu.py::test_fm_tarboton_proportions does on fractals;
    the exact directions have one receiver (rcv bit 0x10 clear), the tilts in between two, and among those is the facet
    whose second receiver wraps from slot 8 to slot 1."""
    wraps = 0
    for name, a, b, hole in PLANES:
        z, got, _ = planes[name]
        exp = orc.port.fm_tarboton(z, ND)
        assert np.array_equal(np.sign(got), np.sign(exp)), name
        assert (ulp_diff_f32(got, exp) <= 1).all(), name
        nrecv = (got[2:-2, 2:-2, 1:] > 0).sum(axis=2)[z[2:-2, 2:-2] != ND]
        if not hole:
            assert (nrecv == (1 if (a, b) in EXACT else 2)).all(), name
        wraps += bool(((got[..., 8] > 0) & (got[..., 1] > 0)).any())
    assert wraps >= 1


@pytest.mark.parametrize("stack_below", STACK_BELOW, ids=lambda s: MODE[s])
def test_dinf_accessor_vs_props_accessor(rd, planes, monkeypatch, stack_below):
    """A: FA_Tarboton (DinfAcc: receiver byte + two shares), B: the generic entry on the engine's own proportions
    (PropsAcc), E: the CPU on the same floats.  Only the order of the f64 sums differs (all terms positive): 1e-12 relative,
    <= 1 ULP after an f32 cast, identical NoData masks -- the tolerance of test_mfd_gpu.py for the same difference."""
    if stack_below is not None:
        monkeypatch.setenv("RDGPU_MFD_STACK_BELOW", stack_below)
    else:
        monkeypatch.delenv("RDGPU_MFD_STACK_BELOW", raising=False)
    for name, _, _, _ in PLANES:
        z, props, E = planes[name]
        A = rd.FlowAccumulation(z, "Dinf", nodata=ND)
        B = rd.FlowAccumFromProps(props)
        for which, got in (("A", A), ("B", B)):
            assert np.array_equal(got == -1, E == -1), (name, which)
            assert np.allclose(got, E, rtol=1e-12, atol=0), (name, which, float(np.abs(got / E - 1).max()))
            assert (ulp_diff_f32(got, E) <= 1).all(), (name, which, int(ulp_diff_f32(got, E).max()))


# ---- 4: the device entries, on the caller's stream --------------------------------------------------------
@pytest.mark.parametrize("name", ["comb_spill", "hubs"])
def test_flow_accumulation_dev_on_a_side_stream(rd, graphs, monkeypatch, name):
    """rdgpu_flow_accumulation_dev_f64 with the weights preloaded in accum, on a non-default stream with work queued before
    and after: exactly the host entry's result (and the oracle's)."""
    import torch

    monkeypatch.delenv("RDGPU_MFD_STACK_BELOW", raising=False)
    p, w, _, ew = graphs[name]
    host = rd.FlowAccumFromProps(p, w)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        tp = torch.from_numpy(p.copy()).cuda(non_blocking=True)
        tp2 = tp * 1.0                                           # (queued work the call must come after)
        acc = torch.from_numpy(w.copy()).cuda(non_blocking=True) + 0.0
        rd.flow_accumulation_dev(tp2, acc)
        rounds = rd.flow_accumulation_rounds()
        acc2 = acc + 0.0                                         # (... and work that must come after it)
    st.synchronize()
    got = acc2.cpu().numpy()
    assert np.array_equal(got, host) and np.array_equal(got, ew), name
    assert rounds >= (2 if name == "comb_spill" else 1)         # (the default schedule stacks a list this short: it spills)


MFD_DEV_METHODS = [("Holmgren", 2.0), ("Freeman", 1.1), ("Quinn", None), ("D4", None)]


@pytest.fixture(scope="module")
def mfd_dem():
    dem = fractal_dem(260, 200, 411)
    dem[90:100, 120:150] = np.float32(-9999)
    dem.setflags(write=False)
    return dem


@pytest.mark.parametrize("method,x", MFD_DEV_METHODS, ids=[m for m, _ in MFD_DEV_METHODS])
def test_fa_mfd_dev_on_a_side_stream(rd, orc, mfd_dem, method, x):
    """rdgpu_fa_mfd_dev_f32 against the host entry (the same device code on the same proportions: only the order of the
    sums differs, 1e-12 relative; D4 is exact) and against the oracle (<= 1 ULP after an f32 cast, the bound of
    test_mfd_gpu.py::test_fa_holmgren_freeman_quinn_d4)."""
    import torch

    nd = np.float32(-9999)
    host = rd.FlowAccumulation(mfd_dem, method, nodata=nd, exponent=x)
    exp = orc.port.fa_mfd(mfd_dem, nd, method, 1.0 if x is None else x)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        z = torch.from_numpy(mfd_dem.copy()).cuda(non_blocking=True)
        z2 = z * 1.0
        acc = torch.ones(z.shape, dtype=torch.float64, device="cuda")
        rd.fa_mfd_dev(z2, nd, method, acc, exponent=x)
        acc2 = acc + 0.0
    st.synchronize()
    got = acc2.cpu().numpy()
    assert np.array_equal(got == -1, host == -1) and np.array_equal(got == -1, exp == -1)
    if method == "D4":
        assert np.array_equal(got, host) and np.array_equal(got, exp)
    else:
        assert np.allclose(got, host, rtol=1e-12, atol=0), float(np.abs(got / host - 1).max())
        u = ulp_diff_f32(got, exp)
        assert (u <= 1).all(), (method, x, int(u.max()))


def test_fa_mfd_dev_refuses_a_wrong_accum(rd, mfd_dem):
    """accum of the wrong shape or dtype: RdgpuError from the wrapper, nothing launched (accum and the launch counter of
    the call before are untouched)."""
    import torch

    nd = np.float32(-9999)
    z = torch.from_numpy(mfd_dem.copy()).cuda()
    good = torch.ones(z.shape, dtype=torch.float64, device="cuda")
    rd.fa_mfd_dev(z, nd, "Quinn", good)
    torch.cuda.synchronize()
    before = rd.flow_accumulation_rounds()
    assert before >= 1
    for bad in (torch.full((z.shape[0], z.shape[1] - 1), 7.0, dtype=torch.float64, device="cuda"),
                torch.full((z.shape[1], z.shape[0]), 7.0, dtype=torch.float64, device="cuda"),
                torch.full(tuple(z.shape), 7.0, dtype=torch.float32, device="cuda"),
                torch.full((z.shape[0], 2 * z.shape[1]), 7.0, dtype=torch.float64, device="cuda")[:, ::2]):
        with pytest.raises(rd.RdgpuError, match="accum must be"):
            rd.fa_mfd_dev(z, nd, "Quinn", bad)
        torch.cuda.synchronize()
        assert bool((bad == 7.0).all()) and rd.flow_accumulation_rounds() == before
    with pytest.raises(rd.RdgpuError):
        rd.fa_mfd_dev(z, nd, "Holmgren", good)                   # the exponent is missing
    with pytest.raises(rd.RdgpuError):
        rd.fa_mfd_dev(z, nd, "Dinf", good)                       # not one of this entry's methods
    with pytest.raises(rd.RdgpuError):
        rd.flow_accumulation_dev(torch.zeros((4, 5, 8), dtype=torch.float32, device="cuda"), good)
