"""Host side of the split-f16 2-D convs in ragged batches (csrc/ragged2d16/, include/satools_hip_ragged2d16.h), CPU only: the entry's
declaration and the conditions on the bounds rows of tests/test_hip_xvector_resnet_ragged16.py (header, binding and table are held
together by tests/test_components_host.py), xvector_resnet.Net.ragged_conv2d_precision and the weights
it packs, asv-eval --resnet-conv2d-ragged, and the float64 calibration of the GPU file's partial fallback."""
import os
import re

import pytest
import torch

import abi_decl
import ref64
import ref64_resnet
import test_hip_xvector_resnet_ragged16 as hr
from satools_amd import _lib, asv_eval, ops, xvector_resnet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "satools_hip_ragged2d16.h"
SOURCE = os.path.join(ROOT, "sa-toolkit_amd", "csrc", "ragged2d16", "conv2d_f16x3_segments.hip")


# ---- what is particular to this component (tests/test_components_host.py holds header, binding, library, build and bounds table together) ----
def test_the_declaration_is_the_one_of_the_issue_names_included():
    args = re.sub(r"\s+", " ", re.search(r"sat_conv2d_f16x3_segments_f32\s*\(([^)]*)\)", abi_decl.code(HEADER)).group(1))
    assert args == ("const float* x, const void* w_split, float w_descale, float* y, const float* ch_scale, const float* ch_shift, int relu, "
                    "const int32_t* in_off, const int32_t* in_len, const int32_t* out_off, int B, int max_len, int Cin, int Cout, int H, int T_in, "
                    "int T_out, int ksize, int stride, int32_t* overflow_flags, void* stream")
    assert callable(ops.conv2d_f16x3_segments)
    assert "satools_hip_ragged2d16.h" in open(os.path.join(ROOT, "include", "satools_hip_ragged2d.h")).read()      # the pointer to the new header


def test_every_ragged2d16_bounds_row_runs_with_and_without_a_broken_table_on_every_instantiation():
    for r in hr.ROWS:
        assert r.shapes and any(s[-1] for s in r.shapes) and any(not s[-1] for s in r.shapes), r.name      # with and without the broken entry
        assert {s[-1] for s in r.shapes} == {"", "in", "out"}                       # on either side
        # every instantiation of the kernel (ksize, stride, 32 | 64 output channels per block at stride 1) has a row
        assert {(k, s, 1 if (cout == 32 or s == 2) else 2) for _, cout, k, s, _, _ in r.shapes} == {(3, 1, 1), (3, 1, 2), (3, 2, 1), (1, 2, 1), (1, 1, 1), (1, 1, 2)}
    assert hr.BROKEN < len(hr.WIDTHS)


def test_the_ragged2d16_family_names_are_not_counted_by_the_other_components_codegen_tests():
    """names the codegen tests of the other components count by substring"""
    assert hr.FAMILIES
    for other in ("conv2d_f16x3_kernel", "conv2d_mfma_kernel", "conv2d_segments_mfma_kernel", "conv2d_stem_kernel"):
        assert not [n for n in hr.FAMILIES if other in n], other


def test_the_gpu_tests_widths_are_the_ones_the_sources_tile_constants_need():
    tile = open(os.path.join(ROOT, "sa-toolkit_amd", "csrc", "conv2d16_tile.h")).read()      # the tile body both forms call
    th = int(re.search(r"constexpr int C16_TH = (\d+);", tile).group(1))
    assert re.search(r"constexpr int TWB = 32 \* NT;", tile)
    text = open(SOURCE).read()
    assert '#include "../conv2d16_tile.h"' in text and "conv2d_f16x3_tile<KS, S, MT, NT>(" in text
    nt = {(int(k), int(s)): int(n) for k, s, _, n in re.findall(r"SAT_R16\((\d), (\d), (\d), (\d)\)", text)}
    assert nt == {(3, 1): 2, (3, 2): 1, (1, 1): 2, (1, 2): 1}                        # 64 output columns per block at stride 1, 32 at stride 2
    tw1, tw2 = 32 * nt[(3, 1)], 32 * nt[(3, 2)]
    assert (th, tw1, tw2) == (hr.TH, hr.TW1, hr.TW2) == (4, 64, 32)
    assert sorted(hr.WIDTHS) == [1, 2, tw2 - 1, tw2, tw2 + 1, tw1 - 1, tw1, tw1 + 1, 2 * tw1 - 1, 2 * tw1, 2 * tw1 + 1] and list(hr.WIDTHS) != sorted(hr.WIDTHS)
    assert {hr.out_widths((w,), 2)[0] for w in (63, 64, 65)} == {tw2, tw2 + 1}
    assert hr.H_CONV == th + 1 and (hr.H_CONV - 1) // 2 + 1 == 3
    assert hr.WIDTHS_256 == (33, 1, 128) and set(hr.WIDTHS_256) <= set(hr.WIDTHS)
    assert hr.CONVS == ((32, 32, 3, 1), (64, 64, 3, 1), (32, 64, 3, 2), (32, 64, 1, 2), (32, 32, 1, 1), (32, 64, 1, 1), (128, 256, 1, 2), (256, 256, 3, 1))
    assert hr.EPILOGUES == ("none", "affine", "affine_relu") and hr.REVERSED_CASE[:4] in hr.CONVS
    assert sorted(hr.NET_SAMPLES) == [1280, 8000, 10079, 10080, 16000, 24123]
    limit = float(re.search(r"#define SAT_CONV2D16_SPLIT_LIMIT ([\d.]+)f", open(os.path.join(ROOT, "include", "satools_hip_conv2d16.h")).read()).group(1))
    assert hr.SPLIT_LIMIT == limit == 65520.0


# ---- ragged_conv2d_precision -------------------------------------------------------------------------------------------------------
def _loaded(Net=None):
    from satools_amd import synthetic
    net = (Net or xvector_resnet.build())(num_speakers=10)
    net.load_state_dict(synthetic.xvector_resnet_state(0, 10), strict=True)
    return net


def test_ragged_conv2d_precision_default_and_environment_variable(monkeypatch):
    monkeypatch.delenv("SATOOLS_AMD_RESNET_CONV2D_RAGGED", raising=False)
    Net = xvector_resnet.build()
    assert Net.ragged_conv2d_precision == "f32" and Net.conv2d_precision in ("f32", "f16x3")
    assert Net.last_split_fallback_rows is None and Net.split_fallbacks == 0
    monkeypatch.setenv("SATOOLS_AMD_RESNET_CONV2D_RAGGED", "f16x3")
    monkeypatch.delenv("SATOOLS_AMD_RESNET_CONV2D", raising=False)
    Net = xvector_resnet.build()
    assert Net.ragged_conv2d_precision == "f16x3" and Net.conv2d_precision == "f32"      # a separate attribute with a variable of its own


def test_ragged_conv2d_precision_packs_the_split_weights_and_is_part_of_the_cache_key(monkeypatch):
    monkeypatch.setattr(_lib, "cache_rebuild_begin", lambda device, had_old: None)
    monkeypatch.setattr(_lib, "cache_rebuild_end", lambda device: None)
    net = _loaded()
    net.conv2d_precision = net.ragged_conv2d_precision = "f32"
    cpu = torch.device("cpu")
    W = net._prepare(cpu)
    convs = lambda W: [e for blk in W["blocks"] for e in (blk["c1"], blk["c2"], blk["sc"]) if e is not None]
    assert len(convs(W)) == 36 and not any("w16" in e for e in convs(W)) and "w16" not in W["stem"]
    assert W["split2d"] is False and W["ragged16"] is False
    assert net._prepare(cpu) is W                                                 # cached
    net.ragged_conv2d_precision = "f16x3"
    W16 = net._prepare(cpu)
    assert W16 is not W                                                           # part of the cache key
    assert W16["split2d"] is False and W16["ragged16"] is True                    # `forward` stays exact f32
    assert all("w16" in e and e["descale"] > 0 and "w" in e for e in convs(W16)) and "w16" not in W16["stem"]
    for e, blk in zip([b["c1"] for b in W16["blocks"]], [b for i in range(4) for b in getattr(net.sequence_network, f"layer{i + 1}")]):
        w16, d = ops.pack_conv2d_weight_f16x3(blk.conv1.weight.detach(), transpose=True)
        assert torch.equal(e["w16"], w16) and e["descale"] == d
    net.ragged_conv2d_precision = "f32"
    net.conv2d_precision = "f16x3"
    W2 = net._prepare(cpu)
    assert W2["split2d"] is True and W2["ragged16"] is False and all("w16" in e for e in convs(W2))
    net.ragged_conv2d_precision = "f64"
    with pytest.raises(_lib.SatError, match=r"ragged_conv2d_precision = 'f64'"):
        net._prepare(cpu)
    net.ragged_conv2d_precision = "f32"
    with pytest.raises(_lib.SatError, match="ragged_conv2d_precision"):          # the split-f16 convs need their weights
        net.embed_segments(torch.zeros(1, 80, 12), None, overflow=torch.zeros(1, dtype=torch.int32))


def test_conv2d_f16x3_segments_checks_its_arguments_before_the_library(monkeypatch):
    def no_library():
        raise AssertionError("the library was reached")

    monkeypatch.setattr(ops, "lib", no_library)
    tab = ops.RaggedLevel([0, 8], [5, 3], 12, seg_off=torch.zeros(2, dtype=torch.int32), seg_len=torch.zeros(2, dtype=torch.int32))
    half = ops.RaggedLevel([0, 8], [3, 2], 12, seg_off=torch.zeros(2, dtype=torch.int32), seg_len=torch.zeros(2, dtype=torch.int32))
    x = torch.zeros(1, 32, 4, 12)
    w16, d = ops.pack_conv2d_weight_f16x3(torch.randn(64, 32, 3, 3))
    sc = torch.ones(64)
    flags = torch.zeros(2, dtype=torch.int32)
    bad = [
        (dict(x=torch.zeros(1, 32, 4, 11)), "columns"), (dict(w=w16.float()), "split weights"), (dict(k=1), "do not fit"), (dict(x=torch.zeros(1, 64, 4, 12)), "do not fit"),
        (dict(sc=torch.ones(32)), "ch_scale"), (dict(d=0.0), "descale"), (dict(d=float("inf")), "descale"), (dict(tout=half), "output table"),
        (dict(s=2), "output table"), (dict(flags=torch.zeros(1, dtype=torch.int32)), "overflow"), (dict(flags=torch.zeros(2, dtype=torch.int64)), "overflow"),
        (dict(out=torch.zeros(1, 64, 4, 11)), "out "),
    ]
    for change, match in bad:
        a = dict(dict(x=x, w=w16, d=d, k=3, s=1, tin=tab, tout=tab, sc=sc, flags=flags, out=None), **change)
        with pytest.raises(_lib.SatError, match=match):
            ops.conv2d_f16x3_segments(a["x"], a["w"], a["d"], a["k"], a["s"], a["tin"], a["tout"], ch_scale=a["sc"], ch_shift=a["sc"], overflow=a["flags"], out=a["out"])
    with pytest.raises(AssertionError, match="the library was reached"):        # and a good call goes on to it
        ops.conv2d_f16x3_segments(x, w16, d, 3, 2, tab, half, ch_scale=sc, ch_shift=sc, overflow=flags)


# ---- asv-eval --resnet-conv2d-ragged -------------------------------------------------------------------------------------------------
def _asv_args(tmp_path):
    return ["--enrolls-wav-scp", str(tmp_path / "e.scp"), "--trails-wav-scp", str(tmp_path / "t.scp"), "--enroll-utt2spk", str(tmp_path / "u2s"),
            "--trials", str(tmp_path / "trials"), "--decode-output", str(tmp_path / "out"), "--device", "cpu"]


def test_asv_eval_option_reaches_the_attribute_and_is_an_error_without_it(monkeypatch, tmp_path, capsys):
    from satools_amd import infer_helper
    seen = {}

    class Model:
        def to(self, device):
            return self

    def test_metrics(model, *a, **kw):
        seen["model"], seen["kw"] = model, kw
        return {"eer": 0.0}

    monkeypatch.setattr(asv_eval, "test_metrics", test_metrics)
    resnet = Model()
    resnet.conv2d_precision, resnet.ragged_conv2d_precision = "f32", "f32"
    monkeypatch.setattr(infer_helper, "load_model", lambda ck: resnet)
    asv_eval.main(["ck"] + _asv_args(tmp_path) + ["--resnet-conv2d-ragged", "f16x3", "--batch-size", "32"])
    assert seen["model"] is resnet and resnet.ragged_conv2d_precision == "f16x3" and resnet.conv2d_precision == "f32" and seen["kw"]["batch_size"] == 32
    resnet.ragged_conv2d_precision = "kept"
    asv_eval.main(["ck"] + _asv_args(tmp_path) + ["--resnet-conv2d", "f16x3"])     # set only when given; --resnet-conv2d governs the other attribute
    assert resnet.ragged_conv2d_precision == "kept" and resnet.conv2d_precision == "f16x3"
    ecapa = Model()
    monkeypatch.setattr(infer_helper, "load_model", lambda ck: ecapa)
    capsys.readouterr()
    with pytest.raises(SystemExit):
        asv_eval.main(["ck"] + _asv_args(tmp_path) + ["--resnet-conv2d-ragged", "f16x3"])
    assert "--resnet-conv2d-ragged" in capsys.readouterr().err and not hasattr(ecapa, "ragged_conv2d_precision")
    with pytest.raises(SystemExit):
        asv_eval.main(["ck"] + _asv_args(tmp_path) + ["--resnet-conv2d-ragged", "f64"])
    capsys.readouterr()
    # the real net has the attribute the option tests for
    assert hasattr(xvector_resnet.build()(), "ragged_conv2d_precision")


# ---- the CPU calibration of the GPU file's partial fallback -------------------------------------------------------------------------------
def _conv_input_peaks(sd, feats):
    """the largest |x| among the inputs of the 36 block convs in the float64 forward (the stem's own input is not staged in f16)"""
    peaks = []
    conv2d = ref64_resnet.conv2d

    def recording(x, w, *a, **kw):
        if torch.as_tensor(w).shape[1] != 1:
            peaks.append(float(torch.as_tensor(x).abs().max()))
        return conv2d(x, w, *a, **kw)

    ref64_resnet.conv2d = recording
    try:
        ref64_resnet.forward(sd, feats)
    finally:
        ref64_resnet.conv2d = conv2d
    assert len(peaks) == 36
    return max(peaks)


def test_the_partial_fallbacks_stem_scale_separates_the_click_from_the_harmonic_utterances_in_float64():
    sd = hr.partial_state()
    wavs = hr.partial_wavs()
    assert len(wavs) == len(hr.PARTIAL_HARMONIC) + 1 and wavs[hr.PARTIAL_CLICK].shape == (hr.PARTIAL_CLICK_SAMPLES,)
    assert int((wavs[hr.PARTIAL_CLICK] != 0).sum()) == 1                           # one click in silence
    fb = sd["preprocessor.MelSpec.mel_scale.fb"].t()
    for i, w in enumerate(wavs):
        feats = ref64.instance_norm(ref64.logmel(w.unsqueeze(0), sd["preprocessor.MelSpec.spectrogram.window"], fb))[0]
        peak = _conv_input_peaks(sd, feats)
        print(f"utterance {i} of {w.shape[0]} samples: largest conv input {peak:.5g} = {peak / hr.SPLIT_LIMIT:.3f} x 65520")
        if i == hr.PARTIAL_CLICK:
            assert peak > 4 * hr.SPLIT_LIMIT, (i, peak)
        else:
            assert peak < hr.SPLIT_LIMIT / 4, (i, peak)
