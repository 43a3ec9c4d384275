"""Host side of the clean and many-to-one anonymizer configs (sa-toolkit_amd/anonymizer_variants.py) and of the generator-input
component (csrc/geninput/, include/satools_hip_geninput.h), CPU only: loading, key lists, the SpeakerCMVN buffer, the float64
restatement against the reference's recorded runs (tests/golden/fx_variants.npz), and the component's constants and refusals (header,
descriptor, binding and build are held together by tests/test_components_host.py)."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import torch

import abi_decl
import ref64_geninput as r64
from satools_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "satools_hip_geninput.h"
VQ, AUG = "bn_tdnnf_600h_vq_48", "bn_tdnnf_600h_aug"
TAGS = {"clean": "clean_hifigan_{}_v1", "m2o": "hifigan_m2o_{}_v1"}
CONFIGS = {"clean": "local/tuning/hifigan_clean.py", "m2o": "local/tuning/hifigan_m2o.py"}


@pytest.fixture(scope="module")
def fx(gold):
    return gold.npz("fx_variants.npz")


# ---- loading -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["clean", "m2o"])
def test_both_configs_load_from_a_checkpoint_file_and_by_synthetic_name(kind, tmp_path, gold):
    """(NotImplementedError at load_model before these configs were built)"""
    import satools_amd
    from satools_amd import synthetic
    state, _ = synthetic.checkpoint(TAGS[kind].format(VQ))
    assert state["base_model_path"] == CONFIGS[kind] and state["task_path"] == "/egs/vc/libritts"
    path = str(tmp_path / "final.pt")
    torch.save(state, path)
    a = satools_amd.load_model(path)
    b = satools_amd.load_model("synthetic:" + TAGS[kind].format(VQ))
    want = gold.json(f"state_dict_keys_hifigan_{kind}.json")
    for net in (a, b):
        sd = net.state_dict()
        assert [[k, list(v.shape), str(v.dtype)] for k, v in sd.items()] == want          # names, order, shapes, dtypes: the reference's
        for name in ("convert", "extract_features", "_forward", "forward", "get_bn", "get_f0", "set_f0", "f0_transformation", "remove_weight_norm"):
            assert callable(getattr(net, name)), name
        assert net.f0_yaapt_opts == {"frame_length": 35.0, "frame_space": 20.0, "nccf_thresh1": 0.25, "tda_frame_length": 25.0}
    assert all(torch.equal(v, b.state_dict()[k]) for k, v in a.state_dict().items())
    assert a.__dict__.get("_precision_check_pending") and not b.__dict__.get("_precision_check_pending")
    if kind == "m2o":
        assert not hasattr(a, "spk") and not hasattr(a, "utt2spk") and a.hifigan.state_dict()["conv_pre.weight_v"].shape == (512, 257, 7)
        assert a.get_spk_id(None) is None
        a.set_f0(torch.ones(1, 3))
        assert a.f0 is not None
    else:
        assert len(a.spk) == 247 and a.hifigan.state_dict()["conv_pre.weight_v"].shape == (512, 256 + 1 + 247, 7)
        assert a.get_spk_id(None, target=a.spk[3]).argmax().item() == 3
        assert [k for k in a.state_dict() if k.startswith("f0_norm.")] == ["f0_norm.model_state_buffer"]
    # the aug (no quantiser) extractor resolves too
    assert satools_amd.load_model("synthetic:" + TAGS[kind].format(AUG)).bn_extractor is not None


def test_other_configs_are_still_refused():
    from satools_amd import infer_helper
    for cfg in ("local/chain/tuning/tdnnf_dp.py", "local/chain/tuning/tdnnf_vq_spkadv.py", "local/tuning/hifigan_other.py"):
        with pytest.raises(NotImplementedError, match="not part of the accelerated path"):
            infer_helper._builder(cfg)
    assert infer_helper._CONFIGS["local/tuning/hifigan_clean.py"] == "anonymizer_clean"
    assert infer_helper._CONFIGS["local/tuning/hifigan_m2o.py"] == "anonymizer_m2o"


@pytest.mark.parametrize("kind", ["clean", "m2o"])
def test_frozen_export_and_convert_padded_are_refused_by_name(kind, tmp_path):
    import satools_amd
    net = satools_amd.load_model("synthetic:" + TAGS[kind].format(VQ))
    with pytest.raises(_lib.SatError, match="frozen export is not built for the '" + CONFIGS[kind]):
        satools_amd.export_frozen(net, str(tmp_path / "x.sat"))
    assert not hasattr(net, "convert_padded")           # the batch job's test for its fused branch
    with pytest.raises(AttributeError, match="convert_padded is not built for the '" + CONFIGS[kind]):
        net.convert_padded
    with pytest.raises(_lib.SatError, match="the model is on the CPU"):
        net._forward(torch.zeros(1, 1, 4), torch.zeros(1, 256, 4)) if kind == "m2o" else net._forward(torch.zeros(1, 1, 4), torch.zeros(1, 256, 4), None)


# ---- SpeakerCMVN -----------------------------------------------------------------------------------------------------------------------------
def test_the_references_buffer_deserialises_to_the_recorded_table(fx):
    from satools_amd import anonymizer_variants as av
    from satools_amd import synthetic
    m = av.SpeakerCMVN()
    buf = torch.zeros(av.STATE_BUFFER_BYTES, dtype=torch.uint8)
    raw = fx["clean/buffer"]
    assert raw.dtype == np.uint8 and raw[0] != 0 and raw[-1] != 0 and len(raw) < av.STATE_BUFFER_BYTES
    buf[:len(raw)] = torch.from_numpy(raw.copy())
    m.load_state_dict({"model_state_buffer": buf})
    table = m.table(247, "cpu")
    assert table.dtype == torch.float32 and np.array_equal(table.numpy(), fx["clean/table"])
    assert int(m.model_state_buffer[0]) == 0 and m.computed and m.keep_zeros               # read once, as the reference marks it
    assert m.table(247, "cpu") is table                                                    # built once per device
    # the synthetic checkpoint's own buffer gives the same table, by the reference's roundings of the seeded moments
    state = synthetic.speaker_cmvn_state(247, 0)
    want = np.asarray([r64.speaker_moments(s["sum"], s["sum_sq"], s["total_frames"]) for s in (state["speaker_stats"][str(i)] for i in range(247))])
    assert np.array_equal(r64.speaker_table(state, 247), fx["clean/table"])
    # (the mean is one rounding of a Python float: equal; the square root is torch's there and numpy's here: one unit in the last place)
    assert np.array_equal(want[:, 0].astype(np.float32), fx["clean/table"][:, 0])
    assert np.all(np.abs(want[:, 1].astype(np.float64) - fx["clean/table"][:, 1]) <= 2.0 ** -23 * fx["clean/table"][:, 1])
    # state_dict() writes the statistics back (a checkpoint saved after the first use keeps them)
    again = av.SpeakerCMVN()
    again.load_state_dict(m.state_dict())
    assert np.array_equal(again.table(247, "cpu").numpy(), fx["clean/table"])
    # a speaker without statistics: the reference's exception, by index string
    m2 = av.SpeakerCMVN()
    m2.load_state_dict({"model_state_buffer": synthetic.speaker_cmvn_buffer(247, 0, skip=(5,))})
    m2.require("4")
    with pytest.raises(RuntimeError) as e:
        m2.require("5")
    assert str(e.value) == str(fx["clean/missing_message"]) and str(fx["clean/missing_type"]) == "RuntimeError"
    assert torch.isnan(m2.table(247, "cpu")[5]).all() and not torch.isnan(m2.table(247, "cpu")[4]).any()
    assert av.one_hot_index_str(torch.tensor([0, 0, 1, 0])) == "2" and av.one_hot_index_str(torch.zeros(4)) == "Value not found"


# ---- the float64 restatement against the reference's runs ------------------------------------------------------------------------------------
@pytest.mark.parametrize("asr,case", [(VQ, "b1"), (VQ, "b2_two_targets"), (AUG, "b2_two_targets")])
def test_ref64_reproduces_the_clean_configs_recorded_rows(fx, asr, case):
    p = f"clean/{asr}/{case}/"
    f0, after, xf0, t = fx[p + "f0"], fx[p + "f0_after"], fx[p + "x_f0"], fx[p + "targets"]
    B, T = xf0.shape
    table = fx["clean/table"]
    bn = np.zeros((B, 1, T), dtype=np.float32)
    bn[:, 0] = fx[p + "x_bn_last"]
    spk = np.eye(247, dtype=np.float32)[t]
    x, norm = r64.generator_input(bn, f0[None], table, [int(t[0])], spk)                  # ONE slice: the first target's row for the batch
    assert np.all(np.abs(after - norm[0]) <= r64.NORM_BOUND * np.abs(norm[0])) and not after[f0 == 0].any()
    assert np.all(np.abs(xf0 - x[:, 1]) <= r64.NORM_BOUND * np.abs(x[:, 1]))
    assert np.array_equal(after[:, r64.interp_index(T, f0.shape[1])], xf0)                # the gather itself: exact
    assert np.array_equal(x[:, 2:], fx[p + "x_spk"].astype(np.float64)) and np.array_equal(x[:, 0], fx[p + "x_bn_last"].astype(np.float64))
    sums = fx[p + "x_sums"]
    assert np.allclose(sums[:, 256], xf0.astype(np.float64).sum(axis=1), rtol=1e-12, atol=1e-9)
    assert np.array_equal(sums[:, 257:], T * spk.astype(np.float64))


def test_ref64_reproduces_the_quantiser_and_the_noise(fx):
    from satools_amd import f0_transforms
    p = f"clean/{VQ}/quant_16_awgn_2/"
    f0, after, xf0, t = fx[p + "f0"], fx[p + "f0_after"], fx[p + "x_f0"], int(fx[p + "targets"][0])
    torch.manual_seed(1234)
    noise = f0_transforms.draw_awgn((1, 1, f0.shape[1]), 2).reshape(1, -1).numpy()
    tr = r64.transform32(after, 16, noise)
    assert np.array_equal(tr[:, r64.interp_index(xf0.shape[1], f0.shape[1])], xf0)
    q = r64.normalise(f0, fx["clean/table"][t, 0], fx["clean/table"][t, 1])
    assert np.all(np.abs(after - q) <= r64.NORM_BOUND * np.abs(q))


def test_ref64_m2o_rows_are_batch_coupled(fx):
    p = f"m2o/{VQ}/b2_set_f0_ignored/"
    track, xf0 = fx[p + "track"].astype(np.float64), fx[p + "x_f0"]
    v = track[track != 0]
    mean, std = v.mean(), np.sqrt(v.var(ddof=1) + 1e-6)                                   # UttCMVN(var_norm=True, keep_zeros=True) over the batch
    want = r64.normalise(track, mean, std)[:, r64.interp_index(xf0.shape[1], track.shape[1])]
    assert np.abs(xf0 - want).max() < 1e-5 and xf0.shape == (2, 30) and fx[p + "x_sums"].shape == (2, 257)
    assert bool((fx[p + "f0_after"] == 123.0).all()) and bool((fx[p + "f0"] == 123.0).all())


# ---- what is particular to this component (tests/test_components_host.py holds header, binding, descriptor, library and build together) ----
def test_geninput_declaration_and_tile_constants():
    assert re.search(r"int sat_generator_input_f32\(const sat_geninput_desc\* d, void\* stream\);", abi_decl.code(HEADER))
    src = open(os.path.join(ROOT, "sa-toolkit_amd", "csrc", "geninput", "generator_input.hip")).read()
    assert int(abi_decl.define(HEADER, "SAT_GENINPUT_TILE")) == 64
    assert "constexpr int GI_TILE = SAT_GENINPUT_TILE;" in src and "constexpr int GI_PITCH = GI_TILE + 1;" in src and "atomic" not in src.lower()


def test_refusals_need_no_gpu():
    lib = _lib.lib()
    assert lib.sat_generator_input_f32(None, None) == -1 and b"generator_input: null descriptor" in lib.sat_last_error()
    d = _lib.GenInputDesc()
    assert lib.sat_generator_input_f32(C.byref(d), None) == -1 and b"generator_input: null pointer" in lib.sat_last_error()


def test_the_existing_kernels_sources_are_restated_not_shared():
    """the statements the new kernel repeats are still the ones of f0_apply_kernel / assemble_kernel (tests/test_hip_geninput.py holds the
    results together on the GPU)"""
    old = re.sub(r"\s+", " ", open(os.path.join(ROOT, "sa-toolkit_amd", "csrc", "bottleneck.hip")).read())
    new = re.sub(r"\s+", " ", open(os.path.join(ROOT, "sa-toolkit_amd", "csrc", "geninput", "generator_input.hip")).read())
    for stmt_old, stmt_new in (("v = v - stats[0]; v = v / stats[1];", "v = v - mean; v = v / std;"),
                               ("rintf(v * (float)quant_bins) / (float)quant_bins", "rintf(v * (float)a.quant_bins) / (float)a.quant_bins"),
                               ("if (v != 0.f) v = v + noise[i];", "if (v != 0.f) v = v + a.noise[i];"),
                               ("const float scale = (float)T_f0 / (float)T;", "const float scale = (float)a.T_f0 / (float)a.T;"),
                               ("int s = (int)floorf((float)t * scale);", "int s = (int)floorf((float)t * scale);")):
        assert stmt_old in old and stmt_new in new, (stmt_old, stmt_new)
