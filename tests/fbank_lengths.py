"""Length catalogue of the fbank tag's end-to-end tests: utterance lengths that sit on the edges of the host plumbing between the
kernels of `TdnnfVqNet` (features -> `_run_layers` -> VQ -> ASR head / `convert()`), each with the property it is there for.

n samples give F = (n + 80) // 160 fbank frames (snip_edges = False; oracle/fbank.py), the fbank kernel takes FB_FRAMES_PER_BLOCK = 4 of
them per block, `pad_input(19)` makes F + 38, and the stack's layers see t_q = F + 36, F + 34, F + 32 frames (three 3-tap layers), then the
context-free stride-2 layer S = ceil((F + 32) / 2) (a 1x1 product on every frame, then `[:, :, ::2]`; bypass `res_toff`, `res_tstride = 2`), then
S - 2 j, j = 1 .. 8, the last of which is the bottleneck: T = S - 16 = ceil(F / 2).  On split planes linearA of a layer is served by the
128 x 256 ring GEMM where `cols256_pad_no_more(t_q)` holds and by the 128 x 128 GEMM elsewhere (csrc/conv1d_api.hip): the rule flips at
t_q = 128 / 129, 256 / 257 and 384 / 385.  The VQ kernel decides 64 frames per block.  The ASR head pads T by 4 + 4 and its 1.5x layer
(`tdnnf_unfold15`, `int(n / 1.5)` bypass frames) leaves its last output frame without a bypass exactly when (T + 8) % 3 == 1; the head
yields (2 (T + 7)) // 3 - 5 frames: one at T = 2, the shortest utterance there is (F = 3, n = 400).

Not reachable below F = 260 (2.6 s), the longest this catalogue goes: the 256-frame blocks of `tdnnf_unfold15` (its output reaches 257 frames
at T = 377, F = 753) and of `assemble` (T = 257, F = 513), and the t_q flip at 384 / 385.  tests/test_hip_bounds.py and
tests/test_hip_small_kernels.py hold those kernels at such sizes on their own.

F0: `convert()` interpolates the YAAPT track of T_f0 = ceil(n / 320) frames (f0.length_dims at the anonymizer's options) to the T bottleneck
frames (`assemble_kernel`, nearest, f32 scale).  Over n in [400, 41600] T_f0 - T takes the values 0 and 1 and no other (T_f0 - 2 T, the
figure the issue of this catalogue names, is just -T or 1 - T): 1 needs an off-grid n, e.g. 160 F + 79 at an even F.  Both are here.

Every entry is (name, n, B, edge, seed0, F, T).  Utterance j of an entry is `synthetic.harm_utterance(seed0 + j, n)`.  The declared
properties are asserted on the CPU by tests/test_fbank_lengths_host.py; the reference's outputs on the catalogue are
tests/golden/fx_fbank_lengths*.npz (tests/golden/make_fixtures.py --only fbank_lengths)."""
from typing import NamedTuple

TAG = "hifigan_bn_tdnnf_600h_vq_48_v1"
FLIP_CAP = 2            # excused VQ index flips per entry below the 5e-3 margin of tests/test_hip_parity.py::_check_extract_bn
PAD, PAD_AFTER = 19, 4
F_MAX_SMALL = 40


class Entry(NamedTuple):
    name: str
    n: int
    B: int
    edge: str
    seed0: int
    F: int              # fbank frames (0: the reference raises)
    T: int              # bottleneck frames

    def seeds(self):
        return list(range(self.seed0, self.seed0 + self.B))

    def wav(self):
        from satools_amd import synthetic
        return synthetic.harm_batch(self.seeds(), self.n)


def fbank_frames(n):
    return (n + 80) // 160 if n >= 400 else 0


def bn_frames(F):
    return -(-F // 2)


def f0_frames(n):
    """frames of the YAAPT track at the anonymizer's options (35 ms frames every 20 ms, the signal padded by 280 samples on either side)"""
    return len(range(280, n + 280, 320))


def stack_tq(F):
    """the frame count each stack layer's linearA (the bottleneck layer: its linearB) works on: tdnn1, tdnnfs.0 .. tdnnfs.20"""
    S = -(-(F + 32) // 2)
    return [F + 36, F + 34, F + 32] + [S - 2 * j for j in range(9)]


def cols256(t_q):
    """`cols256_pad_no_more` of csrc/conv1d_api.hip: linearA on planes goes to the 128 x 256 ring GEMM (True) or the 128 x 128 GEMM (False)"""
    return -(-t_q // 256) * 256 * 8 <= -(-t_q // 128) * 128 * 9


def head_frames(T):
    """output frames of the ASR head behind T bottleneck frames"""
    return (2 * (T + 2 * PAD_AFTER - 1)) // 3 + 1 - 6


def _entries():
    out = []

    def add(name, n, B, edge, seed0=None):
        F = fbank_frames(n)
        out.append(Entry(name, n, B, edge, 900 + 5 * len(out) if seed0 is None else seed0, F, bn_frames(F)))

    for F in range(3, F_MAX_SMALL + 1):
        add(f"F{F}", 400 if F == 3 else 160 * F, 1, "small")
    for F in range(91, 98):
        add(f"F{F}", 160 * F, 1, "dispatch: t_q 127 .. 129 at tdnn1 (F + 36), tdnnfs.0 (F + 34), tdnnfs.2 (F + 32)")
    for F in range(219, 226):
        add(f"F{F}", 160 * F, 1, "dispatch: t_q 255 .. 257 at the three layers before the stride-2 layer; 126 .. 129 at that layer")
    for S in range(130, 144):           # even and odd F in turn
        F = 2 * S - 32 - (S % 2)
        add(f"F{F}", 160 * F, 1, f"dispatch: S = {S}, t_q 127 .. 129 at the layers after the stride-2 layer")
    for F in (126, 127, 129):
        add(f"F{F}", 160 * F, 1, "vq: 63, 64, 65 frames around the VQ kernel's 64-frame block")
    for F in (5, 18, 33, 64, 127, 258):
        add(f"F{F}-80", 160 * F - 80, 1, "off-grid: the smallest n of its F")
        add(f"F{F}+79", 160 * F + 79, 1, "off-grid: the largest n of its F")
    add("off16123", 16123, 1, "off-grid: odd F")
    add("off8192", 8192, 1, "off-grid: odd F")
    add("short399", 399, 1, "too short: below one 25 ms window")
    add("short9", 9, 1, "too short")
    add("B3_F3", 400, 3, "batch: pad_input tiles the last frames of all three utterances; pad 19 longer than the utterance")
    add("B3_F33", 5280, 3, "batch: pad_input tiling at an odd B and an odd F")
    add("B2_F92", 14720, 2, "batch: tdnn1 at the t_q = 128 dispatch flip with a second utterance")
    add("B2_F51", 8160, 2, "batch: convert() of two utterances at an odd F")
    add("B5_F7", 1120, 5, "batch: 19 % 5 != 0, the right-pad tiling walks the rows")
    return out


ENTRIES = _entries()
BY_NAME = {e.name: e for e in ENTRIES}
SMALL = [e for e in ENTRIES if e.edge == "small"]
DISPATCH = [e for e in ENTRIES if e.edge.startswith("dispatch")]
VQ_EDGES = [e for e in ENTRIES if e.edge.startswith("vq")]
OFF_GRID = [e for e in ENTRIES if e.edge.startswith("off-grid")]
TOO_SHORT = [e for e in ENTRIES if e.edge.startswith("too short")]
BATCHES = [e for e in ENTRIES if e.edge.startswith("batch")]
RUNNING = [e for e in ENTRIES if e.F]
#: per-layer activations of the reference are recorded on these (three odd F, three even)
LAYERS = [BY_NAME[n] for n in ("F7", "F8", "F12", "F21", "F33", "F34")]
#: the ASR head: (T + 8) % 3 takes 0, 1 and 2 three times and more; F3 is the smallest T with one output frame; the batches pad_input tiles
ASR = [BY_NAME[n] for n in ("F3", "F5", "F7", "F9", "F12", "F14", "F21", "F33", "F35", "F38", "B3_F3", "B3_F33", "B5_F7")]
#: forward_ragged / convert_padded: utterance 0 of each entry
RAGGED = [("F33", "F12", "F38", "F9"), ("F7", "F40", "F21", "F14")]
#: convert() through the reference's own get_f0: T_f0 - T = 0 (off16123: odd F, off-grid; F40; B2_F51) and 1 (F64+79); F3 raises in the reference
CONVERT = ["off16123", "F64+79", "F40", "B2_F51"]
CONVERT_RAISES = ["F3"]
#: what tests/test_oracle_golden.py runs the CPU oracle on
ORACLE_SUBSET = SMALL + BATCHES
FIXTURES = ("fx_fbank_lengths.npz", "fx_fbank_lengths_edges.npz", "fx_fbank_lengths_layers.npz", "fx_fbank_lengths_convert.npz")
LAYER_NAMES = ["tdnn1"] + [f"tdnnfs.{i}" for i in range(0, 20, 2)]


def convert_targets(spk, B):
    """the target speakers of a recorded convert() call"""
    return spk[3] if B == 1 else [spk[3 + 7 * j] for j in range(B)]


def fixture_part(key):
    """which of FIXTURES a recorded key goes to: each file stays under 500 KB"""
    name, what = key.split("/", 1)
    if what.startswith("convert") or what == "f0":
        return FIXTURES[3]
    if what.startswith("layer/"):
        return FIXTURES[2]
    e = BY_NAME[name]
    return FIXTURES[0] if e in SMALL or e in BATCHES or e in TOO_SHORT else FIXTURES[1]


def fixture(gold):
    """the fixture files as one dict"""
    out = {}
    for name in FIXTURES:
        with gold.npz(name) as f:
            out.update({k: f[k] for k in f.files})
    return out
