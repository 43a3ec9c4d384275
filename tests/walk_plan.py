"""Which block takes which tile: a plain-Python mirror of the grid rules of the persistent kernels (no GPU, no library).

Slot kernels — resblock_pair16_kernel (csrc/pair.hip), mrf16_kernel (mrf.hip), pair32s_kernel and pairw_kernel (pair32s.hip), ups2_kernel
(ups2.hip).  The launcher cuts every utterance into tiles of `width` positions, numbers them utterance by utterance, gives XCD x (= blockIdx.x & 7)
the range [x, x + 1) * per_xcd and launches 8 * nslots blocks, nslots = min(cap, per_xcd); block (xcd, slot) takes tile xcd * per_xcd + slot and
then every nslots-th one of its XCD's range.  A block takes a second tile only when B * ceil(T / width) > 8 * cap.

Ring kernels — conv1d_f16x3_ring16_kernel (conv_ring16.hip), gemm_f16x3_walk16_kernel (gemm_walk16.hip).  n_vb = 8 * n_rt * ceil(n_ct * B / 8)
regions, some of them empty (past the last column tile); `grid` blocks; block i takes regions i, i + grid, ... and in every region the njobs jobs,
in an order that rotates with the region number when the jobs are independent (`locate()` of both kernels).

tests/test_walk_plan_host.py pins every constant and expression mirrored here to the sources, and holds the catalogue of shapes that
tests/test_hip_tile_walk.py runs on the GPU."""

# (family, form) -> (tile width, slot cap per XCD)
SLOT_FORMS = {
    ("pair16", 3): (224, 32 * 4), ("pair16", 7): (224, 32 * 3), ("pair16", 11): (224, 32 * 2),      # FP_TO; 32 * per_cu, per_cu by taps
    ("mrf16", None): (512, 32),                                                                     # MRF_W
    ("pair32s", 8): (240, 32), ("pair32s", 4): (112, 64),                                           # P32<NW>::TQ; NW == 8 ? 32 : 64
    ("pairw", 32): (240, 32), ("pairw", 64): (112, 32),                                             # G::TQ by channels
    ("ups2", 32): (496, 32), ("ups2", 64): (240, 32),                                               # TQ by input channels
}
FORM_KEY = {"pair16": "k", "mrf16": None, "pair32s": "waves", "pairw": "C", "ups2": "C"}
RING_TILES = {4: (256, 160), 2: (128, 320), 1: (64, 384)}      # WR -> (ROWS, COLS) of conv1d_f16x3_ring16_kernel
WALK_TILE = (128, 256)                                         # WK_CO, WK_T of gemm_f16x3_walk16_kernel


def ceil_div(a, b):
    return -(-a // b)


def slot_form(family, **form):
    key = FORM_KEY[family]
    assert set(form) == ({key} if key else set()), (family, form)
    return SLOT_FORMS[(family, form[key] if key else None)]


def slot_grid(family, B, T, **form):
    """(tiles_t, total, per_xcd, nslots) as the launcher computes them"""
    width, cap = slot_form(family, **form)
    tiles_t = ceil_div(T, width)
    total = tiles_t * B
    per_xcd = ceil_div(total, 8)
    return tiles_t, total, per_xcd, max(1, min(cap, per_xcd))


def slot_plan(family, B, T, **form):
    """blocks in blockIdx order, each the ordered list of its (utterance, tile in utterance); a block whose first tile lies past its XCD's
    range returns at once: an empty list"""
    tiles_t, total, per_xcd, nslots = slot_grid(family, B, T, **form)
    blocks = []
    for blk in range(8 * nslots):
        xcd, slot = blk & 7, blk >> 3
        tile_end = min((xcd + 1) * per_xcd, total)
        tile, mine = xcd * per_xcd + slot, []
        while tile < tile_end:
            mine.append((tile // tiles_t, tile % tiles_t))
            tile += nslots          # next = tile + nslots
        blocks.append(mine)
    return blocks


def ring_regions(n_rt, n_ct, B):
    return 8 * n_rt * ceil_div(n_ct * B, 8)


def ring_grid(n_vb, cus, blocks=0):
    """blocks of a ring-conv launch; `blocks`: option convring_blocks as set (rounded down to a multiple of 8 by its setter)"""
    blocks = 0 if blocks < 0 else blocks // 8 * 8
    return min(n_vb, max(8, (min(blocks, cus) if blocks else cus) // 8 * 8))


def walk_grid(n_vb, cus):
    """blocks of a persistent-GEMM launch"""
    return min(n_vb, max(8, cus // 8 * 8))


def ring_plan(n_rt, n_ct, B, njobs=1, rotate=False, grid=8):
    """blocks in blockIdx order, each the ordered list of its (job, utterance or None, row tile, column tile in utterance or None): locate()"""
    n_vb, total = ring_regions(n_rt, n_ct, B), n_ct * B
    assert 1 <= grid <= n_vb
    blocks = []
    for blk in range(grid):
        nreg = (n_vb - blk + grid - 1) // grid
        mine = []
        for k in range(nreg * njobs):
            i, jj = divmod(k, njobs)
            vb = blk + i * grid
            xcd, rest = vb & 7, vb >> 3
            rt, g = rest % n_rt, (rest // n_rt) * 8 + xcd
            j = (jj + vb) % njobs if rotate and njobs > 1 else jj
            mine.append((j, g // n_ct, rt, g % n_ct) if g < total else (j, None, rt, None))
        blocks.append(mine)
    return blocks


def plan(family, B=None, T=None, **form):
    if family in ("ring", "conv_ring16", "gemm_walk16"):
        return ring_plan(B=B, **form)
    return slot_plan(family, B, T, **form)


# ---- what a slot plan exercises -------------------------------------------------------------------------------------------------
def slot_props(family, B, T, **form):
    width, _ = slot_form(family, **form)
    tiles_t = ceil_div(T, width)
    ragged = T % width != 0
    blocks = slot_plan(family, B, T, **form)
    p = {"counts": sorted({len(b) for b in blocks}), "idle_blocks": sum(not b for b in blocks), "walk_steps": 0, "crossings": 0,
         "ragged_nonfirst": 0, "first_tile_after_inner_tile": 0, "ragged_width": T - (tiles_t - 1) * width}
    for b in blocks:
        for (u0, t0), (u1, t1) in zip(b, b[1:]):
            p["walk_steps"] += 1
            p["crossings"] += u1 != u0
            p["ragged_nonfirst"] += ragged and t1 == tiles_t - 1
            p["first_tile_after_inner_tile"] += t1 == 0 and t0 > 0      # left zero padding after a tile that had a real left halo
    covered = sorted(t for b in blocks for t in b)
    assert covered == [(u, t) for u in range(B) for t in range(tiles_t)], "every tile exactly once"
    return p


def nonfirst_tiles(family, B, T, **form):
    return sorted(t for b in slot_plan(family, B, T, **form) for t in b[1:])


def is_crossing(p):
    return 3 in p["counts"] and 2 in p["counts"] and p["crossings"] and p["ragged_nonfirst"] and p["first_tile_after_inner_tile"]


def long_shape(family, **form):
    width, cap = slot_form(family, **form)
    return 1, 8 * cap * width + 1


def even_shape(family, **form):
    """the fewest tiles that are a multiple of 8 * cap and at least twice that, in the shortest utterances that still have a full and a ragged tile"""
    width, cap = slot_form(family, **form)
    return 8 * cap, width + 1


def find_crossing(family, **form):
    """the fewest tiles in all (then the shortest utterances) with an odd B >= 3 and T = m * width + 1 whose plan has every crossing property"""
    width, cap = slot_form(family, **form)
    for total in range(16 * cap + 1, 24 * cap + 1):
        for tiles_t in range(2, total // 3 + 1):
            B = total // tiles_t
            if total % tiles_t or B % 2 == 0 or B < 3:
                continue
            T = (tiles_t - 1) * width + 1
            if is_crossing(slot_props(family, B, T, **form)):
                return B, T
    raise AssertionError("no crossing shape")
