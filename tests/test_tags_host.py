"""All fourteen released tags on the host (no GPU): the seven ASR-BN tags and their `hifigan_` forms resolve and load — as
`synthetic:<tag>` and from a reference-format final.pt — the nets without a quantiser carry exactly the reference's state-dict
entries, and the CPU oracle reproduces the reference fixtures of the new tags (tests/golden/make_tag_fixtures.py)."""
import importlib.util
import os

import pytest
import torch

import satools_amd
from satools_amd import _lib, infer_helper, synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# reference hubconf.py:51-57 -> (model config under egs/asr/librispeech, extractor class, codebook rows or None)
ASR_TAGS = {
    "bn_tdnnf_wav2vec2_vq_48_v1": ("local/chain/tuning/tdnnf_wav2vec2_vq.py", "TdnnfWav2vec2VqNet", 48),
    "bn_tdnnf_wav2vec2_100h_aug_v1": ("local/chain/tuning/tdnnf_wav2vec2.py", "TdnnfWav2vec2Net", None),
    "bn_tdnnf_600h_aug_v1": ("local/chain/tuning/tdnnf.py", "TdnnfNet", None),
    "bn_tdnnf_600h_vq_48_v1": ("local/chain/tuning/tdnnf_vq.py", "TdnnfVqNet", 48),
    "bn_tdnnf_100h_vq_64_v1": ("local/chain/tuning/tdnnf_vq.py", "TdnnfVqNet", 64),
    "bn_tdnnf_100h_vq_256_v1": ("local/chain/tuning/tdnnf_vq.py", "TdnnfVqNet", 256),
    "bn_tdnnf_100h_aug_v1": ("local/chain/tuning/tdnnf.py", "TdnnfNet", None),
}
FBANK_ASR_TAGS = [t for t in ASR_TAGS if "wav2vec2" not in t]
CB_KEY = "tdnnfs.{}.bottleneck_func.quant._embedding.weight"


@pytest.mark.parametrize("tag", list(ASR_TAGS))
def test_asrbn_conf_from_name_for_all_seven_names(tag):
    path, _, rows = ASR_TAGS[tag]
    conf = infer_helper.asrbn_conf_from_name(synthetic.ASR_DIR.format(name=tag[:-len("_v1")]))
    assert conf["base_model_path"] == path and conf["task_path"] == "/egs/asr/librispeech"
    if rows is None:                    # tdnnf.py / tdnnf_wav2vec2.py take neither argument
        assert "codebook_size" not in conf["base_model_args"] and "freeze_encoder" not in conf["base_model_args"]
    else:
        assert conf["base_model_args"]["codebook_size"] == rows


def _check_extractor(ext, tag):
    _, cls, rows = ASR_TAGS[tag]
    assert type(ext).__name__ == cls
    assert ext._has_vq() == (rows is not None)
    keys = list(ext.state_dict())
    last = 2 if "wav2vec2" in tag else 20
    if rows is None:
        assert not any("bottleneck_func" in k for k in keys)
        assert ext._tie_guard(torch.device("cpu")) is None
        for fn in (ext.vq_indices, ext.vq_flip_report):
            with pytest.raises(_lib.SatError, match="no VQ bottleneck"):
                fn(torch.zeros(1, 16000))
    else:
        assert tuple(ext.state_dict()[CB_KEY.format(last)].shape) == (rows, 256)


@pytest.mark.parametrize("tag", list(ASR_TAGS))
def test_all_fourteen_tags_load_synthetic_and_from_a_checkpoint_file(tmp_path, tag):
    """`synthetic:<tag>`, `synthetic:hifigan_<tag>` and a reference-format final.pt of both, written to disk (the wav2vec2 files are
    1.3 GB each: removed as soon as they are read)"""
    models = {}
    for t in (tag, "hifigan_" + tag):
        state, _ = synthetic.checkpoint(t)
        model = models[t] = satools_amd.load_model("synthetic:" + t)             # (the same draw: synthetic keeps the last one)
        _check_extractor(getattr(model, "bn_extractor", model), tag)
        p = tmp_path / t
        p.mkdir()
        torch.save(state, p / "final.pt")
        del state
        try:
            m = satools_amd.load_model(str(p / "final.pt"))
        finally:
            os.unlink(p / "final.pt")
        assert type(m).__name__ == type(model).__name__ and list(m.state_dict()) == list(model.state_dict())
        assert all(torch.equal(v, model.state_dict()[k]) for k, v in m.state_dict().items())
        _check_extractor(getattr(m, "bn_extractor", m), tag)
        del m
    ext, net = models[tag], models["hifigan_" + tag]
    assert list(ext.state_dict()) == list(net.bn_extractor.state_dict())
    assert (ext.padding, ext.padding_after) == ((3, 4) if "wav2vec2" in tag else (19, 4))


def test_state_dicts_of_the_nets_without_a_quantiser_match_the_reference(gold):
    """key, shape and dtype lists of the reference's tdnnf.py / tdnnf_wav2vec2.py nets"""
    for tag, file in (("bn_tdnnf_600h_aug_v1", "state_dict_keys_fbank_novq.json"), ("bn_tdnnf_100h_aug_v1", "state_dict_keys_fbank_novq.json"),
                      ("bn_tdnnf_wav2vec2_100h_aug_v1", "state_dict_keys_w2v2_novq.json")):
        conf = infer_helper.asrbn_conf_from_name(synthetic.ASR_DIR.format(name=tag[:-len("_v1")]))
        from satools_amd.anonymizer import SimpleNamespace
        with torch.device("meta"):
            net = infer_helper._builder(conf["base_model_path"])(SimpleNamespace(**conf["base_model_args"]))(**conf["base_model_params"])
        mine = [[k, list(v.shape), str(v.dtype)] for k, v in net.state_dict().items()]
        assert mine == gold.json(file), tag
        # the VQ twin's list minus its quantiser entries
        twin = gold.json("state_dict_keys_w2v2.json" if "wav2vec2" in tag else "state_dict_keys_fbank.json")
        assert mine == [[e[0][len("bn_extractor."):]] + e[1:] for e in twin if e[0].startswith("bn_extractor.") and "bottleneck_func" not in e[0]]


def test_other_asr_configs_are_still_refused(tmp_path):
    state, _ = synthetic.checkpoint("bn_tdnnf_600h_aug_v1")
    for cfg in ("local/chain/tuning/tdnnf_dp.py", "local/chain/tuning/tdnnf_spkadv.py"):
        state["base_model_path"] = cfg
        p = tmp_path / "final.pt"
        torch.save(state, p)
        with pytest.raises(NotImplementedError):
            satools_amd.load_model(str(p))


def test_hubconf_passes_every_tag_through(monkeypatch):
    spec = importlib.util.spec_from_file_location("hubconf", os.path.join(ROOT, "hubconf.py"))
    hub = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(hub)
    seen = []

    class M:
        def eval(self):
            return self

    monkeypatch.setattr(satools_amd, "load_model", lambda f, option_args=None: seen.append(f) or M())
    for tag in ASR_TAGS:
        assert tag in hub.asr_bn_extractor.__doc__ and "hifigan_" + tag in hub.anonymization.__doc__
        hub.asr_bn_extractor("synthetic:" + tag)
        hub.anonymization("synthetic:hifigan_" + tag)
        hub.anonymization("hifigan_" + tag)
    assert seen == [f for tag in ASR_TAGS for f in ("synthetic:" + tag, "synthetic:hifigan_" + tag, os.path.join("hifigan_" + tag, "final.pt"))]


def test_new_vq_entry_points_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "satools_hip.h")).read()
    lib = _lib.lib()
    for name in ("sat_vq_argmin_gather_tiled_f32", "sat_vq_argmin_gather_tiled_tie_f32"):
        assert name + "(" in header and hasattr(lib, name) and name in _lib.symbols("core")
    assert lib.sat_abi_version() == 8


def test_oracle_reproduces_the_fixture_of_the_net_without_a_quantiser(gold):
    from oracle import tdnnf as otd
    fx = gold.npz("fx_tags.npz")
    from oracle import convert as oconv
    for tag in ("hifigan_bn_tdnnf_600h_aug_v1", "hifigan_bn_tdnnf_100h_aug_v1"):          # the `100h` name draws the same weights
        state, _ = synthetic.checkpoint(tag)
        sd, _ = oconv.split_state_dict(state["base_model_state_dict"])
        assert not any("bottleneck_func" in k for k in sd)
        aux = {}
        bn = otd.extract_bn_fbank(sd, synthetic.harm_batch([0, 1], 80000), aux=aux)
        assert not aux and bn.shape == (2, 250, 256)
        err = (bn.permute(0, 2, 1)[:, ::8, :] - torch.from_numpy(fx["bn_tdnnf_600h_aug/harm01_80000/bn_sub"])).abs().max()
        bn1 = otd.extract_bn_fbank(sd, synthetic.harm_batch([0], 8000))
        err1 = (bn1.permute(0, 2, 1) - torch.from_numpy(fx["bn_tdnnf_600h_aug/harm0_8000/bn"])).abs().max()
        print(f"{tag}: oracle vs reference fixture, max abs error {float(err):.2e} (5 s x 2), {float(err1):.2e} (0.5 s)")
        assert err < 2e-4 and err1 < 2e-4


def test_oracle_reproduces_the_indices_of_the_256_code_fixture(gold):
    from oracle import tdnnf as otd
    fx = gold.npz("fx_tags.npz")
    from oracle import convert as oconv
    state, _ = synthetic.checkpoint("hifigan_bn_tdnnf_100h_vq_256_v1")
    sd, _ = oconv.split_state_dict(state["base_model_state_dict"])
    assert tuple(sd[CB_KEY.format(20)].shape) == (256, 256)
    for name, seeds in (("harm01_80000", [0, 1]), ("harm3to10_80000", list(range(3, 11)))):
        margin = torch.from_numpy(fx[f"bn_tdnnf_100h_vq_256/{name}/margin"])
        sure = margin > 5e-3
        assert float((~sure).float().mean()) <= 0.01              # at most 1 % of the frames are left out of the comparison
        aux = {}
        bn = otd.extract_bn_fbank(sd, synthetic.harm_batch(seeds, 80000), aux=aux)
        agree = aux["idx"] == torch.from_numpy(fx[f"bn_tdnnf_100h_vq_256/{name}/idx"]).long()
        print(f"bn_tdnnf_100h_vq_256 {name}: {int((~sure).sum())} of {sure.numel()} frames under the margin, "
              f"{int((~agree).sum())} indices differ, {len(set(aux['idx'].flatten().tolist()))} codes in use")
        assert agree[sure].all()
        if name == "harm01_80000":
            ref = torch.from_numpy(fx[f"bn_tdnnf_100h_vq_256/{name}/bn_sub"])
            assert (bn.permute(0, 2, 1)[:, ::8, :] - ref).permute(0, 2, 1)[agree].abs().max() < 2e-4


def test_bench_reaches_load_model_for_the_new_tags():
    """bench.py reads the guard's figures with getattr(ext, "vq_tie_sigmas", None) and ext.__dict__.get("tie_stats"): a net without a
    quantiser has the class attribute, no tie_stats of its own, and no guard"""
    net = satools_amd.load_model("synthetic:hifigan_bn_tdnnf_600h_aug_v1")
    ext = net.bn_extractor
    assert getattr(ext, "vq_tie_sigmas", None) is not None and ext.__dict__.get("tie_stats") is None
    assert ext._tie_calibration(torch.device("cpu")) is None
