"""Host side of the ragged x-vector batches (csrc/ragged/, include/satools_hip_ragged.h), CPU only: the packed layout and the tile table
(ops.ragged_layout / ragged_tiles), the grouping of asv_eval's extraction with a stub model that records its calls, and the shapes of
tests/test_hip_xvector_ragged.py against the kernels' constants (header, binding and bounds table are held together by
tests/test_components_host.py)."""
import os
import re

import numpy as np
import pytest
import torch

import test_hip_xvector_ragged as hr
from satools_amd import _lib, asv_eval, ops, pipeline

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "satools_hip_ragged.h"


# ---- the packed layout -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frames", [(1,), (4, 63, 64, 65, 127, 128, 129, 257), (2, 2, 2), (6, 1, 1, 5, 3), tuple(range(1, 40)), (70000, 3)])
def test_ragged_layout_follows_the_documented_rule(frames):
    off, length, t_tot = ops.ragged_layout(frames)
    assert off.dtype == length.dtype == np.int32 and length.tolist() == list(frames) and off[0] == 0
    ends = [int(o) + int(n) for o, n in zip(off, length)]
    nxt = off.tolist()[1:] + [t_tot]
    for e, o in zip(ends, nxt):
        assert o == -(-(e + 2) // 4) * 4                                          # off_{i+1} = round_up(off_i + T_i + 2, 4); T_tot = off_B
        assert 2 <= o - e <= 5                                                    # at least 2 gap columns, the last segment included
    assert all(b > a for a, b in zip(off.tolist(), nxt)) and all(o % 4 == 0 for o in nxt)
    text = open(os.path.join(ROOT, "include", HEADER)).read()
    assert "off_{i+1} = round_up(off_i + T_i + 2, 4)" in text and "T_tot = off_B" in text
    assert (ops.RAGGED_GAP, ops.RAGGED_ALIGN) == (2, 4)
    assert int(re.search(r"#define SAT_RAGGED_MAX_SEGMENTS (\d+)", text).group(1)) == ops.RAGGED_MAX_SEGMENTS == 1024


def test_ragged_layout_and_tiles_refuse_and_count():
    for bad in ([], [3, 0, 2], [-1], [5] * 1025):
        with pytest.raises(_lib.SatError):
            ops.ragged_layout(bad)
    assert ops.ragged_layout([5] * 1024)[2] == 1024 * 8
    tiles, n64, n128 = ops.ragged_tiles((7, 64, 65, 128, 129, 193))
    assert tiles.dtype == np.int32 and tiles.shape == (n64 + n128, 2) and (n64, n128) == (1 + 1 + 2 + 2 + 3 + 4, 1 + 1 + 1 + 1 + 2 + 2)
    assert tiles[:n64].tolist() == [[0, 0], [1, 0], [2, 0], [2, 64], [3, 0], [3, 64], [4, 0], [4, 64], [4, 128], [5, 0], [5, 64], [5, 128], [5, 192]]
    assert tiles[n64:].tolist() == [[0, 0], [1, 0], [2, 0], [3, 0], [4, 0], [4, 128], [5, 0], [5, 128]]


# ---- the grouping of the extraction ------------------------------------------------------------------------------------------------
class _Stub:
    """records its calls; the 'x-vector' of an utterance is (its sample count, its first sample)"""

    def __init__(self):
        self.single, self.batches = [], []

    def __call__(self, wav, target=None):
        self.single.append(int(wav.shape[0]))
        return (None, None), torch.tensor([[float(wav.shape[0]), float(wav[0])]])


class _RaggedStub(_Stub):
    def extract_batch(self, wavs):
        self.batches.append([int(w.shape[0]) for w in wavs])
        return torch.tensor([[float(w.shape[0]), float(w[0])] for w in wavs])


@pytest.fixture(scope="module")
def toy(tmp_path_factory):
    d = tmp_path_factory.mktemp("ragged_toy")
    lengths = {"e1": 1600, "e2": 3300, "e3": 800, "b1": 2400, "t1": 1000, "t2": 4100, "t3": 1700}
    for k, (name, n) in enumerate(lengths.items()):
        pipeline.save_pcm16(d / (name + ".wav"), torch.full((1, n), (k + 1) / 16.0), 16000)
    enroll = {n: str(d / (n + ".wav")) for n in ("e1", "e2", "b1", "e3")}
    trials = {n: str(d / (n + ".wav")) for n in ("t1", "b1", "t2", "t3")}          # b1 is in both lists
    return enroll, trials, lengths


def _check_vectors(enroll, trial, toy):
    e_scp, t_scp, lengths = toy
    assert list(enroll) == list(e_scp) and list(trial) == list(t_scp)
    for u, v in {**enroll, **trial}.items():
        assert v.shape == (2,) and int(v[0]) == lengths[u] and float(v[1]) == (list(lengths).index(u) + 1) / 16.0, u
    assert trial["b1"] is enroll["b1"] or torch.equal(trial["b1"], enroll["b1"])


def test_groups_of_up_to_batch_size_in_scp_order_and_shared_utterances_once(toy):
    m = _RaggedStub()
    enroll, trial = asv_eval.extract_xvectors(m, toy[0], toy[1], torch.device("cpu"), batch_size=3)
    assert m.single == [] and m.batches == [[1600, 3300, 2400], [800, 1000, 4100], [1700]]      # enrolment order, then the new trial utterances
    _check_vectors(enroll, trial, toy)
    m = _RaggedStub()
    asv_eval.extract_xvectors(m, toy[0], toy[1], torch.device("cpu"), batch_size=64)
    assert m.batches == [[1600, 3300, 2400, 800, 1000, 4100, 1700]]


def test_the_max_frames_cap_cuts_a_group_and_a_long_utterance_goes_alone(toy):
    m = _RaggedStub()
    # frames: 11, 21, 16, 6, 7, 26, 11
    enroll, trial = asv_eval.extract_xvectors(m, toy[0], toy[1], torch.device("cpu"), batch_size=4, max_frames=40)
    assert m.batches == [[1600, 3300], [2400, 800, 1000], [4100, 1700]]
    _check_vectors(enroll, trial, toy)
    m = _RaggedStub()
    asv_eval.extract_xvectors(m, toy[0], toy[1], torch.device("cpu"), batch_size=4, max_frames=20)
    assert m.batches == [[1600], [3300], [2400], [800, 1000], [4100], [1700]]      # 21 and 26 frames exceed the cap: calls of their own


def test_batch_size_one_never_calls_extract_batch(toy):
    m = _RaggedStub()
    enroll, trial = asv_eval.extract_xvectors(m, toy[0], toy[1], torch.device("cpu"))
    assert m.batches == [] and m.single == [1600, 3300, 2400, 800, 1000, 4100, 1700]
    _check_vectors(enroll, trial, toy)
    assert trial["b1"] is enroll["b1"]


def test_a_model_without_extract_batch_extracts_one_per_call_and_says_so_once(toy, caplog):
    asv_eval._logged_no_batch.discard("_Stub")
    m = _Stub()
    with caplog.at_level("WARNING"):
        enroll, trial = asv_eval.extract_xvectors(m, toy[0], toy[1], torch.device("cpu"), batch_size=8)
        asv_eval.extract_xvectors(m, toy[0], toy[1], torch.device("cpu"), batch_size=8)
    assert m.single == [1600, 3300, 2400, 800, 1000, 4100, 1700] * 2
    _check_vectors(enroll, trial, toy)
    assert len([r for r in caplog.records if "no extract_batch" in r.getMessage()]) == 1


def test_command_line_and_test_metrics_carry_the_options(monkeypatch, tmp_path, capsys):
    import inspect
    from satools_amd import infer_helper
    sig = inspect.signature(asv_eval.test_metrics)
    assert sig.parameters["batch_size"].default == 1 and sig.parameters["max_frames"].default == 65536

    class Model:
        def to(self, device):
            return self

    seen = []
    monkeypatch.setattr(asv_eval, "test_metrics", lambda model, *a, **k: seen.append(k) or {"eer": 0.0})
    monkeypatch.setattr(infer_helper, "load_model", lambda path: Model())
    args = ["ck", "--enrolls-wav-scp", "e", "--trails-wav-scp", "t", "--enroll-utt2spk", "u", "--trials", "l", "--decode-output", str(tmp_path)]
    asv_eval.main(args)
    assert "batch_size" not in seen[-1] and "max_frames" not in seen[-1]          # the default: the present call, unchanged
    asv_eval.main(args + ["--batch-size", "32"])
    assert seen[-1]["batch_size"] == 32 and seen[-1]["max_frames"] == 65536
    asv_eval.main(args + ["--batch-size", "8", "--max-frames", "9000"])
    assert seen[-1]["batch_size"] == 8 and seen[-1]["max_frames"] == 9000
    for bad in (["--batch-size", "0"], ["--max-frames", "0"]):
        with pytest.raises(SystemExit):
            asv_eval.main(args + bad)
    capsys.readouterr()
    with pytest.raises(SystemExit):
        asv_eval.main(["--help"])
    assert "--batch-size N" in capsys.readouterr().out


def test_extract_batch_checks_its_arguments_before_any_device_call(monkeypatch):
    from satools_amd import synthetic, xvector
    net = xvector.build()(num_speakers=10)
    net.load_state_dict(synthetic.xvector_state(0, 10), strict=True)
    assert callable(net.extract_batch) and callable(net.embed_segments)
    with pytest.raises(_lib.SatError, match="no CPU fallback"):
        net.extract_batch([torch.zeros(8000)])
    with pytest.raises(_lib.SatError, match="no CPU fallback"):
        net.extract_batch((torch.zeros(2, 8000), [8000, 700]))
    with pytest.raises(_lib.SatError, match="1-D"):
        net.extract_batch([torch.zeros(2, 8000)])
    with pytest.raises(_lib.SatError, match="lengths"):
        net.extract_batch((torch.zeros(2, 8000), [8000, 9000]))
    with pytest.raises(_lib.SatError, match="empty"):
        net.extract_batch([])


# ---- what is particular to this component (tests/test_components_host.py holds header, binding, library, build and bounds table together) ----
def test_ops_has_the_wrappers_of_the_ragged_entries():
    for name in ("ragged_layout", "ragged_tiles", "melspec_logmel_segments", "instnorm_segments", "row_mean_segments", "se_gate_add_segments",
                 "attentive_stats_segments", "res2_chain_segments"):
        assert callable(getattr(ops, name)), name


def test_the_gpu_tests_shapes_straddle_the_wave_and_the_chains_centres():
    csrc = os.path.join(ROOT, "sa-toolkit_amd", "csrc")
    text = open(os.path.join(csrc, "ragged", "xvector_ragged.hip")).read()      # the segment kernels: lookups, exits, pointers
    rows = open(os.path.join(csrc, "xvector.hip")).read()                         # the row kernels
    tile = open(os.path.join(csrc, "xvector_tile.h")).read()                      # the bodies and constants both share
    body = open(os.path.join(csrc, "xvector_chain_body.h")).read()                # the chain's statements, included by both
    # the reductions stride by the 64 lanes of a wave: seven loops over t in the shared row bodies (three of InstanceNorm, one of the row
    # mean, three of the attentive statistics), two in the gap zeroing of instnorm_segments_kernel, none with another stride anywhere
    assert [len(re.findall(r"t \+= 64\)", s)) for s in (tile, text, rows, body)] == [7, 2, 0, 0] and hr.WAVE == 64
    assert not re.findall(r"\bt \+= (?!64\))", tile + text + rows + body)
    assert {hr.WAVE - 1, hr.WAVE, hr.WAVE + 1, 2 * hr.WAVE - 1, 2 * hr.WAVE, 2 * hr.WAVE + 1} <= set(hr.FRAMES)
    assert sorted(hr.FRAMES) == [4, 63, 64, 65, 127, 128, 129, 257] and list(hr.FRAMES) != sorted(hr.FRAMES)
    # the chain's centres: W - 2 HALO columns of a window of 64 NT, NT = 2 and 3
    halo = int(re.search(r"constexpr int R2_MARG = \d+, R2_HALO = (\d+);", tile).group(1))
    assert "TT = W - 2 * R2_HALO" in body and "constexpr int W = 64 * NT" in body
    assert text.count('#include "../xvector_chain_body.h"') == 1 and rows.count('#include "xvector_chain_body.h"') == 1
    centres = sorted(64 * nt - 2 * halo for nt in (2, 3))
    for src, kernel in ((text, "res2_chain_segments_kernel"), (rows, "res2_chain_kernel")):
        assert f"launch_res2_chain<2>({kernel}<2>," in src and f"launch_res2_chain<3>({kernel}<3>," in src
    assert centres == sorted(hr.CENTRES) == [64, 128]
    # one below / at / one above the 64-column centre; at / one above the 128-column centre (127 is not among the lengths: 65 ends inside its first
    # tile like 127 would); 193 = one column into a fourth 64-column and a second 128-column tile; 7 < the halo
    assert {63, 64, 65} <= set(hr.CHAIN_FRAMES) and {128, 129} <= set(hr.CHAIN_FRAMES) and 193 == 3 * 64 + 1 and min(hr.CHAIN_FRAMES) < halo
    assert sorted(hr.CHAIN_FRAMES) == [7, 63, 64, 65, 128, 129, 193] and set(hr.CHAIN_CASES) == {(7, 2), (7, 3), (7, 4), (3, 1)}
    assert all(n * d <= halo for n, d in hr.CHAIN_CASES)
    # the front end: frames = 1 + n // 160, four frames per block, 513 samples the shortest
    assert int(re.search(r"constexpr int XV_FPB = (\d+);", tile).group(1)) == 4 and int(re.search(r"constexpr int XV_HOP = (\d+);", tile).group(1)) == ops.XV_HOP
    assert "ceil_div(1 + n_max / XV_HOP, XV_FPB)" in text and "ceil_div(frames, XV_FPB)" in rows          # both grids are sized by them
    assert sorted(1 + n // ops.XV_HOP for n in hr.FRONT_SAMPLES) == [4, 5, 63, 64, 65, 151] and min(hr.FRONT_SAMPLES) == ops.XV_MIN_SAMPLES
    assert sorted(hr.NET_SAMPLES) == [641, 8000, 10079, 10080, 16000, 24123]
    # every channel count leaves a block of four waves ending inside a row of segments, and the gate kernel's channel group is straddled
    cpb = int(re.search(r"constexpr int RG_CPB = (\d+);", text).group(1))
    assert set(hr.CHANNELS) == {5, 8} and cpb in hr.CHANNELS and any(c % cpb for c in hr.CHANNELS)
