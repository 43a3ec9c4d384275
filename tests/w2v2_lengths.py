"""Length catalogue of the wav2vec2 tag's end-to-end tests: utterance lengths that sit on the edges of the host plumbing
between the kernels of `TdnnfWav2vec2VqNet.w2v2_features`, each with the property it is there for.

The feature extractor maps n samples to frame counts L0..L6 (`_fe_lens`: a 10-tap stride-5 conv, four 3-tap and two 2-tap
stride-2 convs), L6 = T = (n - 400) // 320 + 1 for n >= 400.  The LayerNorm before each stride-2 conv writes its L_i
frames as an even and an odd phase of (L_i + 1) // 2 slots each; an odd L_i leaves the odd phase's last slot zero, an even
one fills it, and the 3-tap convs (one wrapped 1x1 product) read "the even phase one frame later" up to that slot.  Which
of the two happens at each of the six layers is the PARITY PATTERN (L0 % 2, .., L5 % 2) of a length: 64 patterns, and
n = 1040 + 5 k, k = 0..63, walks all of them at T = 3.

Behind the extractor T decides: the LayerNorm kernel works in blocks of 32 frames, the residual stream and the VQ in
pitches / blocks of 64, the fused attention in blocks of 256 keys, and the positional conv's twelve shifted 11-tap pieces
read windows [t + 11 s - 64, t + 11 s - 54] that lie wholly outside a sequence of T < 57 frames for the late pieces.

Every entry is (name, n, B, edge).  Utterance j of an entry is `synthetic.harm_utterance(seed0 + j, n)`.  The declared
properties are asserted on the CPU by tests/test_w2v2_lengths_host.py; the reference's outputs on the catalogue are
tests/golden/fx_w2v2_lengths*.npz (tests/golden/make_fixtures.py --only w2v2_lengths)."""
from typing import NamedTuple

TAG = "hifigan_bn_tdnnf_wav2vec2_vq_48_v1"
NOVQ_TAG = "hifigan_bn_tdnnf_wav2vec2_100h_aug_v1"
PARITY_N0, PARITY_STEP, PARITY_COUNT, PARITY_T = 1040, 5, 64, 3
FLIP_CAP = 2            # excused VQ index flips per entry, split-f16 mode (tests/test_hip_robust.py: the long-utterance test's cap)


class Entry(NamedTuple):
    name: str
    n: int
    B: int
    edge: str
    seed0: int
    T: int              # final frame count (0: the reference raises)

    def seeds(self):
        return list(range(self.seed0, self.seed0 + self.B))

    def wav(self):
        from satools_amd import synthetic
        return synthetic.harm_batch(self.seeds(), self.n)


def frames(n):
    return (n - 400) // 320 + 1 if n >= 400 else 0


def _entries():
    out = []

    def add(name, n, B, edge):
        out.append(Entry(name, n, B, edge, 700 + 5 * len(out), frames(n)))

    for k in range(PARITY_COUNT):
        add(f"parity{k:02d}", PARITY_N0 + PARITY_STEP * k, 1, "parity")
    for T, edge in ((1, "one frame: every positional-conv piece but s = 5 reads outside the sequence"),
                    (2, "two frames: pad_input's right pad (3) longer than the utterance"),
                    (3, "three frames"),
                    (31, "LayerNorm 32-frame block - 1"), (32, "LayerNorm 32-frame block"), (33, "LayerNorm 32-frame block + 1"),
                    (63, "64-frame pitch and VQ block - 1"), (64, "64-frame pitch: tp == T"), (65, "64-frame pitch + 1"),
                    (255, "attention 256-key block - 1"), (256, "attention 256-key block, tp == T"), (257, "attention: a second key block of one key")):
        add(f"T{T}", 400 + 320 * (T - 1), 1, edge)
    add("off1044", 1044, 1, "off-grid: the frames of 1040, four samples in no frame")
    add("off16123", 16123, 1, "off-grid: n % 5 == 3")
    for T in (2, 32, 64, 256):
        add(f"T{T}+159", 400 + 320 * (T - 1) + 159, 1, "off-grid: T-edge shifted by +159 samples")
    add("short399", 399, 1, "too short: L6 == 0")
    add("short9", 9, 1, "too short: shorter than conv 0's kernel")
    add("B3_T2", 720, 3, "batch: pad_input tiles the last frames of all three utterances; pad longer than the utterance")
    add("B3_T33", 10640, 3, "batch: pad_input tiling at an odd B")
    add("B2_T64", 20560, 2, "batch: tp == T with a second utterance")
    add("B2_T32", 10320, 2, "batch: convert() of two utterances at a LayerNorm block edge")
    return out


ENTRIES = _entries()
BY_NAME = {e.name: e for e in ENTRIES}
PARITY = [e for e in ENTRIES if e.edge == "parity"]
T_EDGES = [e for e in ENTRIES if e.name.startswith("T") and "+" not in e.name]
OFF_GRID = [e for e in ENTRIES if e.edge.startswith("off-grid")]
TOO_SHORT = [e for e in ENTRIES if e.edge.startswith("too short")]
BATCHES = [e for e in ENTRIES if e.edge.startswith("batch")]
WHOLE = T_EDGES + OFF_GRID                       # the whole-extractor sweep of the GPU test
#: convert() through the reference's own get_f0, recorded as "<entry>/convert": (entry, stored sample step: every 4th of the longest)
CONVERT = [("off16123", 1), ("T64", 4), ("B2_T32", 1)]


def convert_targets(spk, B):
    """the target speakers of a recorded convert() call"""
    return spk[3] if B == 1 else [spk[3 + 7 * j] for j in range(B)]


#: what tests/test_oracle_w2v2.py runs the CPU oracle on: the T <= 65 edges, the B = 3 batches, eight parity entries
ORACLE_SUBSET = [e for e in T_EDGES if e.T <= 65] + [e for e in BATCHES if e.B == 3] + PARITY[5::8]
FIXTURES = ("fx_w2v2_lengths.npz", "fx_w2v2_lengths_parity.npz", "fx_w2v2_lengths_batches.npz")


def fixture(gold):
    """the three fixture files as one dict (the parity set, and the batches with the convert() waveforms, are files of their own:
    each stays under 500 KB)"""
    out = {}
    for name in FIXTURES:
        with gold.npz(name) as f:
            out.update({k: f[k] for k in f.files})
    return out


def parity_pattern(fe_lens):
    """(L0 % 2, .., L5 % 2) of the seven frame counts `_fe_lens` returns"""
    return tuple(t % 2 for t in fe_lens[:6])
