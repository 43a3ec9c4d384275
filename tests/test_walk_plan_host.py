"""tests/walk_plan.py held against the sources, and the catalogue of shapes at which a block of a persistent kernel takes a second tile
(tests/test_hip_tile_walk.py runs them on the GPU).  No GPU here: the plan is arithmetic.

The pins: every tile width, slot cap and grid expression that walk_plan.py mirrors is read out of csrc/ by regex.  A change to one of
them fails here first, and the catalogue below then needs revisiting: its shapes are the smallest that have their property UNDER THESE
CONSTANTS, committed as literals.

The catalogue, per slot kernel and form:
    long      B = 1, T = 8 * cap * width + 1: one utterance longer than the grid.  Slot 0 of XCDs 0..6 takes two tiles, XCD 7's range is
              short (six of its blocks return at once), the last tile is one column wide
    crossing  odd B >= 3, T = m * width + 1: some block takes 3 tiles and some 2; walk steps change utterance; a block's non-first tile is
              the ragged last tile of an utterance; a block's non-first tile is the first tile of an utterance after a tile with a real
              left halo.  The fewest tiles (then the smallest m) that have all of it: walk_plan.find_crossing
    even      B * tiles_t = 2 * 8 * cap exactly: every block takes two tiles
and for the ring conv under convring_blocks = 8 the entries of RING below."""
import os
import re

import pytest

import walk_plan as wp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sa-toolkit_amd", "csrc")
REVISIT = "a constant or grid rule of a persistent kernel changed: tests/walk_plan.py and the catalogue of tests/test_walk_plan_host.py need revisiting"

# (family, form) -> {kind: (B, T)}
SLOT = {
    ("pair16", 3): {"long": (1, 229377), "crossing": (683, 449), "even": (1024, 225)},
    ("pair16", 7): {"long": (1, 172033), "crossing": (53, 6273), "even": (768, 225)},
    ("pair16", 11): {"long": (1, 114689), "crossing": (205, 897), "even": (512, 225)},
    ("mrf16", None): {"long": (1, 131073), "crossing": (171, 1025), "even": (256, 513)},
    ("pair32s", 8): {"long": (1, 61441), "crossing": (171, 481), "even": (256, 241)},
    ("pair32s", 4): {"long": (1, 57345), "crossing": (205, 449), "even": (512, 113)},
    ("pairw", 32): {"long": (1, 61441), "crossing": (171, 481), "even": (256, 241)},
    ("pairw", 64): {"long": (1, 28673), "crossing": (171, 225), "even": (256, 113)},
    ("ups2", 32): {"long": (1, 126977), "crossing": (171, 993), "even": (256, 497)},
    ("ups2", 64): {"long": (1, 61441), "crossing": (171, 481), "even": (256, 241)},
}
# ring conv under convring_blocks = 8: name -> (n_rt, n_ct, B, njobs, rotate)
RING = {
    "two regions, seven of the second round empty": (1, 3, 3, 1, False),
    "three regions per block, one utterance": (1, 17, 1, 1, False),
    "two row tiles": (2, 3, 3, 1, False),
    "three rotating jobs": (1, 3, 3, 3, True),
}
RING_BLOCKS = 8


def form_kw(family, f):
    return {wp.FORM_KEY[family]: f} if wp.FORM_KEY[family] else {}


def _src(name):
    return re.sub(r"\s+", " ", open(os.path.join(CSRC, name)).read())


def _find(name, pattern, n=None):
    """the groups of every match of `pattern` (a regex over the source with runs of white space collapsed) in csrc/<name>"""
    got = re.findall(pattern, _src(name))
    assert got and (n is None or len(got) == n), f"csrc/{name}: {pattern!r} found {len(got)} times. {REVISIT}"
    return got


def _has(name, *lines):
    for line in lines:
        _find(name, re.escape(line))


# ---- the pins ---------------------------------------------------------------------------------------------------------------------
def test_tile_widths_are_the_ones_in_the_sources():
    assert int(_find("pair.hip", r"constexpr int FP_TO = (\d+);", 1)[0]) == wp.SLOT_FORMS[("pair16", 3)][0] == wp.SLOT_FORMS[("pair16", 7)][0] \
        == wp.SLOT_FORMS[("pair16", 11)][0], REVISIT
    assert int(_find("mrf.hip", r"constexpr int MRF_W = (\d+);", 1)[0]) == wp.SLOT_FORMS[("mrf16", None)][0], REVISIT
    w8, w4 = _find("pair32s.hip", r"static constexpr int TQ = NW == 8 \? (\d+) : (\d+);", 1)[0]
    assert (int(w8), int(w4)) == (wp.SLOT_FORMS[("pair32s", 8)][0], wp.SLOT_FORMS[("pair32s", 4)][0]), REVISIT
    w32, w64 = _find("pair32s.hip", r"static constexpr int TQ = C == 32 \? (\d+) : (\d+);", 1)[0]
    assert (int(w32), int(w64)) == (wp.SLOT_FORMS[("pairw", 32)][0], wp.SLOT_FORMS[("pairw", 64)][0]), REVISIT
    for u32, u64 in _find("ups2.hip", r"constexpr int TQ = CIN == 32 \? (\d+) : (\d+);", 2):          # the kernel and its launcher
        assert (int(u32), int(u64)) == (wp.SLOT_FORMS[("ups2", 32)][0], wp.SLOT_FORMS[("ups2", 64)][0]), REVISIT
    co, t = _find("gemm_walk16.hip", r"constexpr int WK_CO = (\d+), WK_T = (\d+),", 1)[0]
    assert (int(co), int(t)) == wp.WALK_TILE, REVISIT
    _has("gemm_walk16.hip", "A.n_rt = ceil_div(A.rows_g, WK_CO);", "A.n_ct = ceil_div(A.T, WK_T);", "t.co_b = rt * CO_B;", "t.q_b = (g - t.b * A.n_ct) * T_B;",
         "CO_B = WK_CO, T_B = WK_T,")
    # the ring conv: ROWS / COLS per WR from the kernel's own expressions
    _has("conv_ring16.hip", "constexpr int WC = 8 / WR, MT = 4, NT = WR == 1 ? 3 : 5, ROWS = 64 * WR, COLS = 16 * NT * WC;",
         "constexpr int WC = 8 / WR, NT = WR == 1 ? 3 : 5, ROWS = 64 * WR, COLS = 16 * NT * WC,",
         "A.n_rt = ceil_div(a[0].rows_g, ROWS);", "A.n_ct = ceil_div(a[0].T_q, COLS);", "t.co_b = rt * ROWS;", "t.q_b = (g - t.b * A.n_ct) * COLS;")
    for wr, tile in wp.RING_TILES.items():
        assert (64 * wr, 16 * (3 if wr == 1 else 5) * (8 // wr)) == tile, REVISIT
    # which WR a launch gets: 256 x 160 for more than 128 rows unless convring_wr says 128 x 320 (bit 0: f16x3, bit 1: F8); the upsampler form 256 x 160
    _has("conv_ring16.hip", "return a[0].rows_g > 128 && !(g_convring_wr & 1) ? launch_convring<4>(a, njobs, rotate, B, s) : launch_convring<2>(a, njobs, rotate, B, s);",
         "a[0].rows_g > 128 && !(g_convring_wr & 2) ? launch_convring<4, -1, true>(a, njobs, rotate, B, s) : launch_convring<2, -1, true>(a, njobs, rotate, B, s);",
         "launch_convring<4, (int)UPS_MASK_K8>(&a, 1, 0, B, s) : launch_convring<4, 0>(&a, 1, 0, B, s);", "constexpr unsigned UPS_MASK_K8 = 0x30cu;")


def test_slot_caps_and_the_slot_walk_are_the_ones_in_the_sources():
    k11, k7, k3 = (int(v) for v in _find("pair.hip", r"const int per_cu = KS == 11 \? (\d+) : KS == 7 \? (\d+) : (\d+);", 1)[0])
    assert {3: 32 * k3, 7: 32 * k7, 11: 32 * k11} == {k: wp.SLOT_FORMS[("pair16", k)][1] for k in (3, 7, 11)}, REVISIT
    _has("pair.hip", "p.pp_tiles_t = ceil_div(p.T_q, FP_TO);", "p.pp_total = p.pp_tiles_t * B;", "p.pp_per_xcd = ceil_div(p.pp_total, 8);",
         "p.pp_nslots = std::max(1, std::min(32 * per_cu, p.pp_per_xcd));", "dim3 grid(8 * p.pp_nslots, 1, 1);",
         "const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;", "const int tile_end = min((xcd + 1) * p.pp_per_xcd, p.pp_total);",
         "int tile = xcd * p.pp_per_xcd + slot;", "if (tile >= tile_end) return;", "const int next = tile + p.pp_nslots;", "const bool more = next < tile_end;",
         "const int b = __builtin_amdgcn_readfirstlane(tile / p.pp_tiles_t);", "const int t0 = (tile - b * p.pp_tiles_t) * FP_TO;")
    walk = ("const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;", "const int tile_end = min((xcd + 1) * p.per_xcd, p.total);", "int tile = xcd * p.per_xcd + slot;",
            "if (tile >= tile_end) return;", "const int next = tile + p.nslots;", "const bool more = next < tile_end;",
            "const int b = __builtin_amdgcn_readfirstlane(tile / p.tiles_t);")
    grid = ("p.total = p.tiles_t * p.B;", "p.per_xcd = ceil_div(p.total, 8);")
    _has("mrf.hip", *walk, *grid, "p.tiles_t = ceil_div(p.T, MRF_W);", "p.nslots = std::max(1, std::min(32, p.per_xcd));", "dim3 grid(8 * p.nslots, 1, 1);",
         "const int t0 = (tile - b * p.tiles_t) * MRF_W;")
    assert wp.SLOT_FORMS[("mrf16", None)][1] == 32
    _has("ups2.hip", *walk, *grid, "p.tiles_t = ceil_div(p.T, TQ);", "p.nslots = std::max(1, std::min(32, p.per_xcd));", "dim3(8 * p.nslots)",
         "const int q0 = (tile - b * p.tiles_t) * TQ;")
    assert wp.SLOT_FORMS[("ups2", 32)][1] == wp.SLOT_FORMS[("ups2", 64)][1] == 32
    # pair32s_kernel walks like the others; pairw_kernel counts its tiles first (n_my) and steps tile0 + step * nslots
    _has("pair32s.hip", *walk, *grid, "p.tiles_t = ceil_div(p.T, P32<NW>::TQ);", "p.nslots = std::max(1, std::min(NW == 8 ? 32 : 64, p.per_xcd));",
         "p.tiles_t = ceil_div(p.T, G::TQ);", "p.nslots = std::max(1, std::min(32, p.per_xcd));", "const int tile0 = xcd * p.per_xcd + slot;",
         "if (tile0 >= tile_end) return;", "const int n_my = (tile_end - tile0 + p.nslots - 1) / p.nslots;", "const int tile = tile0 + step * p.nslots;",
         "const int p0 = (tile - b * p.tiles_t) * TQ;")
    _find("pair32s.hip", re.escape("dim3(8 * p.nslots)"), 2)
    assert (wp.SLOT_FORMS[("pair32s", 8)][1], wp.SLOT_FORMS[("pair32s", 4)][1]) == (32, 64) and wp.SLOT_FORMS[("pairw", 32)][1] == wp.SLOT_FORMS[("pairw", 64)][1] == 32
    # which kernel a fused step gets (the forms of the catalogue): C = 64 and 7 / 11 taps at C = 32 wave-specialised, 3 taps at C = 32 by pair32s_waves
    _has("pair32s.hip", "if (a.cin_g == 64) return launch_pairw<64, 3>(p, s);", "if (a.ksize == 7) return launch_pairw<32, 7>(p, s);",
         "if (a.ksize == 11) return launch_pairw<32, 11>(p, s);", "if (g_pair32s_waves == 4) {")


def test_the_staged_halos_are_the_ones_in_the_sources():
    """what tests/test_hip_tile_walk.py leaves out at the edges of a crop of the long utterance"""
    assert int(_find("pair.hip", r"constexpr int FP_OFF = (\d+);", 1)[0]) == 16, REVISIT
    assert int(_find("mrf.hip", r"constexpr int MRF_HP = (\d+);", 1)[0]) == 64, REVISIT
    _has("ups2.hip", "the image holds q0 - 1 .. q0 + TQ")


def test_the_ring_grids_and_locate_are_the_ones_in_the_sources():
    _has("conv_ring16.hip", "A.total = A.n_ct * B;", "A.n_vb = 8 * A.n_rt * ceil_div(A.total, 8);",
         "const int grid = std::min(A.n_vb, std::max(8, (g_convring_blocks ? std::min(g_convring_blocks, cu_count()) : cu_count()) / 8 * 8));",
         "void convring_set_blocks(int v) { g_convring_blocks = v < 0 ? 0 : v / 8 * 8; }", "A.rotate = rotate && njobs > 1;",
         "const int nreg = (A.n_vb - (int)blockIdx.x + (int)gridDim.x - 1) / (int)gridDim.x;", "const int ntiles = nreg * njobs;",
         "const int i = __builtin_amdgcn_readfirstlane(k / njobs), jj = k - i * njobs;", "const int vb = (int)blockIdx.x + i * (int)gridDim.x;",
         "const int xcd = vb & 7, rest = vb >> 3;", "const int rt = __builtin_amdgcn_readfirstlane(rest % A.n_rt);",
         "const int g = __builtin_amdgcn_readfirstlane((rest / A.n_rt) * 8 + xcd);", "t.j = A.rotate ? __builtin_amdgcn_readfirstlane((jj + vb) % njobs) : jj;",
         "t.b = g < A.total ? __builtin_amdgcn_readfirstlane(g / A.n_ct) : -1;")
    _has("gemm_walk16.hip", "A.total = A.n_ct * B;", "A.n_vb = 8 * A.n_rt * ceil_div(A.total, 8);",
         "const int grid = std::min(A.n_vb, std::max(8, walk_cu_count() / 8 * 8));",
         "const int nreg = (A.n_vb - (int)blockIdx.x + (int)gridDim.x - 1) / (int)gridDim.x;", "const int ntiles = nreg * njobs;",
         "const int i = __builtin_amdgcn_readfirstlane(k / njobs);", "t.j = k - i * njobs;", "const int vb = (int)blockIdx.x + i * (int)gridDim.x;",
         "const int xcd = vb & 7, rest = vb >> 3;", "const int rt = __builtin_amdgcn_readfirstlane(rest % A.n_rt);",
         "const int g = __builtin_amdgcn_readfirstlane((rest / A.n_rt) * 8 + xcd);", "t.b = g < A.total ? __builtin_amdgcn_readfirstlane(g / A.n_ct) : -1;")
    for cus in range(8, 513, 8):
        for n_vb in (8, 16, 24, cus, cus + 8, 2 * cus, 5 * cus):
            assert wp.ring_grid(n_vb, cus) == wp.walk_grid(n_vb, cus) == min(n_vb, cus)
            assert wp.ring_grid(n_vb, cus, 8) == wp.ring_grid(n_vb, cus, 15) == 8
            assert wp.ring_grid(n_vb, cus, 1024) == min(n_vb, cus) and wp.ring_grid(n_vb, cus, 7) == min(n_vb, cus)      # (7 rounds down to 0: the default)
    assert wp.ring_grid(640, 308) == 304 and wp.ring_grid(640, 5) == 8          # a CU count that is no multiple of 8; never fewer than one block per XCD


# ---- the catalogue ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,f", list(SLOT), ids=lambda v: str(v))
def test_slot_catalogue_has_the_properties_it_is_there_for(family, f):
    kw = form_kw(family, f)
    width, cap = wp.slot_form(family, **kw)
    shapes = SLOT[(family, f)]
    # long
    B, T = shapes["long"]
    assert (B, T) == wp.long_shape(family, **kw) == (1, 8 * cap * width + 1)
    blocks = wp.slot_plan(family, B, T, **kw)
    assert len(blocks) == 8 * cap
    for xcd in range(7):
        assert len(blocks[xcd]) == 2 and all(len(blocks[8 * s + xcd]) == 1 for s in range(1, cap))          # slot 0 of XCDs 0..6 takes two tiles
    assert [len(blocks[8 * s + 7]) for s in range(cap)] == [1] * (cap - 6) + [0] * 6                         # XCD 7's range is short
    p = wp.slot_props(family, B, T, **kw)
    assert p["ragged_width"] == 1 and p["walk_steps"] == 7 and p["idle_blocks"] == 6
    # crossing
    B, T = shapes["crossing"]
    assert B % 2 == 1 and B >= 3 and T % width == 1 and (B, T) == wp.find_crossing(family, **kw)
    p = wp.slot_props(family, B, T, **kw)
    assert p["counts"] == [1, 2, 3] and p["crossings"] > 0 and p["ragged_nonfirst"] > 0 and p["first_tile_after_inner_tile"] > 0 and wp.is_crossing(p)
    # even
    B, T = shapes["even"]
    assert (B, T) == wp.even_shape(family, **kw)
    tiles_t, total, per_xcd, nslots = wp.slot_grid(family, B, T, **kw)
    assert total == 2 * 8 * cap and nslots == cap and per_xcd == 2 * cap
    p = wp.slot_props(family, B, T, **kw)
    assert p["counts"] == [2] and p["crossings"] > 0 and p["ragged_nonfirst"] > 0
    # what the GPU tests compare against walks nowhere: sub-batches of at most 8 * cap tiles
    for kind in ("crossing", "even"):
        B, T = shapes[kind]
        sub = sub_batch(family, B, T, **kw)
        assert sub >= 1 and wp.slot_props(family, sub, T, **kw)["counts"] in ([1], [0, 1]) and wp.slot_props(family, sub, T, **kw)["walk_steps"] == 0
    # the crops of the long utterance cover every non-first tile, each well inside its crop
    B, T = shapes["long"]
    seen = set()
    for a, L in crops(family, **kw):
        assert a % width == 0 and L <= 8 * cap * width and a + L <= T
        assert wp.slot_props(family, 1, L, **kw)["walk_steps"] == 0
        seen.update(t for t in range(a // width + 1, (a + L) // width - 1 + (a + L == T)))
    assert {t for _, t in wp.nonfirst_tiles(family, B, T, **kw)} <= seen


def sub_batch(family, B, T, **kw):
    """utterances per unwalked sub-batch: B_sub * tiles_t <= 8 * cap"""
    width, cap = wp.slot_form(family, **kw)
    return min(B, 8 * cap // wp.ceil_div(T, width))


def crops(family, **kw):
    """(a, L) of the crops of the long utterance: the tile before each non-first tile, the tile itself and the one after it"""
    width, cap = wp.slot_form(family, **kw)
    B, T = wp.long_shape(family, **kw)
    out = []
    for _, t in wp.nonfirst_tiles(family, B, T, **kw):
        a = (t - 1) * width
        out.append((a, min(3 * width, T - a)))
    return out


def test_every_family_walks_three_tiles_across_an_utterance_onto_a_ragged_tile():
    for (family, f), shapes in SLOT.items():
        p = wp.slot_props(family, *shapes["crossing"], **form_kw(family, f))
        assert max(p["counts"]) == 3 and p["crossings"] and p["ragged_nonfirst"], (family, f)


def test_ring_catalogue_has_the_properties_it_is_there_for():
    def P(name, grid=RING_BLOCKS):
        n_rt, n_ct, B, njobs, rot = RING[name]
        return wp.plan("ring", n_rt=n_rt, n_ct=n_ct, B=B, njobs=njobs, rotate=rot, grid=grid), wp.ring_regions(n_rt, n_ct, B)
    blocks, n_vb = P("two regions, seven of the second round empty")
    assert n_vb == 16 and len(blocks) == 8 and all(len(b) == 2 for b in blocks)
    assert sum(b[1][1] is None for b in blocks) == 7 and all(b[0][1] is not None for b in blocks)
    assert blocks[0] == [(0, 0, 0, 0), (0, 2, 0, 2)]          # tile 8 = utterance 2's ragged last column tile
    blocks, n_vb = P("three regions per block, one utterance")
    assert n_vb == 24 and all(len(b) == 3 for b in blocks) and blocks[0] == [(0, 0, 0, 0), (0, 0, 0, 8), (0, 0, 0, 16)]
    assert sorted(t[3] for b in blocks for t in b if t[1] is not None) == list(range(17))
    blocks, n_vb = P("two row tiles")
    assert n_vb == 32 and all(len(b) == 4 for b in blocks) and [t[2] for t in blocks[0]] == [0, 1, 0, 1]
    assert blocks[0][:2] == [(0, 0, 0, 0), (0, 0, 1, 0)] and blocks[0][2:] == [(0, 2, 0, 2), (0, 2, 1, 2)]          # both row tiles of a column tile in one block
    # ... so a block takes more than three tiles, crosses into another utterance and ends on the ragged last column tile (column tile 2 of 3)
    assert any(len(b) >= 3 and b[0][1] != b[2][1] and b[2][3] == 2 for b in blocks)
    blocks, n_vb = P("three rotating jobs")
    assert n_vb == 16 and all(len(b) == 6 for b in blocks)
    assert any(b[0][1] != b[3][1] and b[3][3] == 2 for b in blocks)
    assert {b[0][0] for b in blocks} == {0, 1, 2}          # the blocks start on different jobs
    for b in blocks:
        assert sorted(t[0] for t in b[:3]) == sorted(t[0] for t in b[3:]) == [0, 1, 2] and len({t[1:] for t in b[:3]}) == 1
    # every tile of every job exactly once, whatever the grid
    for name, (n_rt, n_ct, B, njobs, rot) in RING.items():
        for grid in (8, 16, wp.ring_regions(n_rt, n_ct, B)):
            got = sorted(t for b in P(name, min(grid, wp.ring_regions(n_rt, n_ct, B)))[0] for t in b if t[1] is not None)
            assert got == sorted((j, u, rt, ct) for j in range(njobs) for u in range(B) for rt in range(n_rt) for ct in range(n_ct)), name


def test_the_kernel_level_shapes_of_the_older_tests_walk_nowhere():
    """what made this catalogue necessary: the most tiles any case of tests/test_hip_parity.py or of the table of tests/test_hip_bounds.py gives
    these kernels — every block takes one tile.  (If a later table has a shape that walks, this assertion can go.)"""
    import test_hip_bounds as hb
    most = {("pair16", 3): 24, ("pair16", 7): 24, ("pair16", 11): 24, ("mrf16", None): 18, ("pair32s", 8): 36, ("ups2", 32): 14, ("ups2", 64): 14}
    for (family, f), tiles in most.items():
        width, cap = wp.slot_form(family, **form_kw(family, f))
        assert tiles <= 8 * cap
        assert wp.slot_props(family, tiles, width, **form_kw(family, f))["walk_steps"] == 0
    table = {("pair16", 7): hb.times(224) + [(3, 1061)], ("pair16", 11): hb.times(224), ("mrf16", None): hb.times(512) + [(3, 60), (1, 11), (3, 513)],
             ("pair32s", 8): hb.times(240), ("pair32s", 4): hb.times(112), ("pairw", 32): hb.times(240), ("pairw", 64): hb.times(112),
             ("ups2", 32): hb.times(496), ("ups2", 64): hb.times(240)}
    for (family, f), shapes in table.items():
        for B, T in shapes:
            assert wp.slot_props(family, B, T, **form_kw(family, f))["walk_steps"] == 0, (family, f, B, T)
    # the ring kernels: between 16 and 40 regions, fewer than any CU count they run on: one region per block
    for rows, cols in ((128, 320), (256, 160)):
        for B, T in hb.times(cols):
            n_vb = wp.ring_regions(1, wp.ceil_div(T, cols), B)
            assert n_vb <= 40 and wp.ring_grid(n_vb, 64) == n_vb
