#!/usr/bin/env python3
"""Golden fixtures of the tags beyond the first three — the nets without a quantiser (`bn_tdnnf_600h_aug`, `bn_tdnnf_100h_aug`,
`bn_tdnnf_wav2vec2_100h_aug`) and the 256-code VQ (`bn_tdnnf_100h_vq_256`) — made by IMPORTING THE REFERENCE in the build
container, like make_fixtures.py (whose helpers this script uses).  Run from the repo root:
    python tests/golden/make_tag_fixtures.py [--only keys conditioning fbank w2v2]

The reference nets are built through the reference's own `build(args)` (tdnnf.py, tdnnf_wav2vec2.py, tdnnf_vq.py with
codebook_size = 256, hifigan.py) and loaded strictly with the synthetic state dict.  Data only is written:
  state_dict_keys_fbank_novq.json, state_dict_keys_w2v2_novq.json    key / shape / dtype lists of the reference nets
  conditioning_bn_tdnnf_100h_vq_256.npz                              BatchNorm statistics + a 256-row codebook: 256 of the calibration
                                                                     batch's 1 000 bottleneck frames (randperm seed 0)
  fx_tags.npz                                                        extract_bn of harm_batch([0, 1], 80000) for bn_tdnnf_600h_aug
                                                                     (every 8th frame row, as fx_tdnnf.npz) and bn_tdnnf_100h_vq_256
                                                                     (+ idx, margin); extract_bn of harm_batch([0, 1], 16000) for
                                                                     bn_tdnnf_wav2vec2_100h_aug
  fx_e2e_<asr name>.npz                                              convert() on the inputs and targets of fx_e2e.npz
The *_aug names take their conditioning (BatchNorm statistics only) from their VQ twins' committed files
(synthetic._CONDITIONING_ALIAS): the calibration of the fbank net is recomputed here and asserted equal."""
import argparse
import json
import os

import numpy as np

from make_fixtures import GOLD, build_reference_model, setup_reference

MARGIN = 5e-3          # frames whose two best codes are closer than this are left out of index comparisons ...
MARGIN_CAP = 0.01      # ... at most this share of the frames (asserted when the fixture is written)


def calibrate_rows(net, calib_wavs, vq_layer, rows):
    """make_fixtures.calibrate with the number of codebook rows as an argument (None: a net without a quantiser): one forward with the
    BatchNorm modules in train mode / momentum 1 (running stats := batch stats), then a codebook of `rows` frames of the bottleneck
    layer's own input (randperm seed 0).  -> the conditioning dict"""
    import torch
    bx = net.bn_extractor
    bns = [m for m in bx.modules() if isinstance(m, torch.nn.BatchNorm1d)]
    for m in bns:
        m.train()
        m.momentum = 1.0
    zs = []
    layer = bx.tdnnfs[vq_layer]
    h = layer.tdnn.linearB.register_forward_hook(lambda m, i, o: zs.append(o.detach()))
    with torch.no_grad():
        bx.extract_bn(calib_wavs.clone())
    h.remove()
    for m in bns:
        m.eval()
        m.momentum = 0.1
    z = zs[0].reshape(-1, zs[0].shape[-1])
    if rows is not None:
        sel = torch.randperm(z.shape[0], generator=torch.Generator().manual_seed(0))[:rows]
        layer.bottleneck_func.quant._embedding.weight.data.copy_(z[sel].clone())
    cond = {}
    for k, v in bx.state_dict().items():
        used = k.startswith("tdnn1.") or (k.startswith("tdnnfs.") and int(k.split(".")[1]) <= vq_layer)
        if used and (k.endswith("running_mean") or k.endswith("running_var") or k.endswith("_embedding.weight")):
            cond[k] = v.numpy().copy()
    return cond, z.shape[0]


def reference_net(ref, asr_name, conditioning="auto"):
    """(reference Net of hifigan_<asr_name> with the synthetic weights loaded strictly, the checkpoint dict)"""
    from satools_amd import synthetic
    tag = "hifigan_" + asr_name + "_v1"
    net = build_reference_model(ref, asr_name)
    state, mine = synthetic.checkpoint(tag, conditioning=conditioning)
    res = net.load_state_dict(state["base_model_state_dict"], strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert list(net.state_dict()) == list(mine.state_dict())
    net.eval()
    return net, state


def keys_of(module):
    return [[k, list(v.shape), str(v.dtype)] for k, v in module.state_dict().items()]


def convert_fixture(net, path):
    """the three plain convert() cases of fx_e2e.npz"""
    import torch
    from satools_amd import synthetic
    spk, out = net.spk, {}
    with torch.no_grad():
        out["harm0_80000_str"] = net.convert(synthetic.harm_batch([0], 80000), target=spk[3]).numpy()
        out["harm01_80000_list"] = net.convert(synthetic.harm_batch([0, 1], 80000), target=[spk[3], spk[10]]).numpy()
        out["rand0_16000_str"] = net.convert(synthetic.rand_batch(0, 1, 16000), target=spk[7]).numpy()
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) <= 1058046 + 4096, "larger than the largest fixture under tests/golden"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", nargs="*", default=None)
    a = ap.parse_args()
    want = lambda name: a.only is None or name in a.only
    ref = setup_reference()
    import torch
    torch.set_num_threads(8)
    import satools  # noqa: F401  (the reference)
    from satools_amd import synthetic

    fx_path = os.path.join(GOLD, "fx_tags.npz")
    fx = dict(np.load(fx_path)) if os.path.exists(fx_path) else {}
    calib = torch.cat([synthetic.harm_batch(range(100, 108), 32000), synthetic.rand_batch(5, 2, 32000) * 2 - 1], 0)

    if want("keys") or want("fbank"):
        aug = "bn_tdnnf_600h_aug"
        net, state = reference_net(ref, aug, conditioning=None)
        if want("keys"):
            json.dump(keys_of(net.bn_extractor), open(os.path.join(GOLD, "state_dict_keys_fbank_novq.json"), "w"))
            assert not any("bottleneck_func" in k for k in net.bn_extractor.state_dict())
        if want("fbank"):
            # the BatchNorm statistics of the net without the quantiser are those its VQ twin's committed file holds
            cond, _ = calibrate_rows(net, calib, vq_layer=20, rows=None)
            twin = dict(np.load(synthetic.conditioning_path(aug)))
            for k, v in cond.items():
                if k.startswith("tdnn1.") or int(k.split(".")[1]) < 20:
                    assert np.array_equal(v, twin[k]), k
            net, state = reference_net(ref, aug)
            wav = synthetic.harm_batch([0, 1], 80000)
            with torch.no_grad():
                bn = net.get_bn(wav)                                       # [2, 256, 250]
            fx[f"{aug}/harm01_80000/bn_sub"] = bn[:, ::8, :].numpy()
            fx[f"{aug}/harm0_8000/bn"] = net.get_bn(synthetic.harm_batch([0], 8000)).detach().numpy()
            convert_fixture(net, os.path.join(GOLD, f"fx_e2e_{aug}.npz"))
            # the `100h` name draws the same weights: one fixture serves both
            net2, state2 = reference_net(ref, "bn_tdnnf_100h_aug")
            assert all(torch.equal(v, state2["base_model_state_dict"][k]) for k, v in state["base_model_state_dict"].items())

    vq = "bn_tdnnf_100h_vq_256"
    cond_path = os.path.join(GOLD, f"conditioning_{vq}.npz")
    if want("conditioning") or (want("fbank") and not os.path.exists(cond_path)):
        net, _ = reference_net(ref, vq, conditioning=None)
        cond, frames = calibrate_rows(net, calib, vq_layer=20, rows=256)
        assert frames == 1000 and cond["tdnnfs.20.bottleneck_func.quant._embedding.weight"].shape == (256, 256)
        np.savez(cond_path, **cond)
    if want("fbank"):
        net, _ = reference_net(ref, vq)
        for name, wav in [("harm01_80000", synthetic.harm_batch([0, 1], 80000)), ("harm3to10_80000", synthetic.harm_batch(range(3, 11), 80000))]:
            acts = {}
            h = net.bn_extractor.tdnnfs[20].bottleneck_func.quant.register_forward_hook(
                lambda m, i, o: acts.update(idx=o[5].detach(), dist=o[4].detach()))
            with torch.no_grad():
                bn = net.get_bn(wav)
            h.remove()
            B = wav.shape[0]
            srt = acts["dist"].sort(1)[0]
            margin = (srt[:, 1] - srt[:, 0]).reshape(B, -1)
            low = int((margin <= MARGIN).sum())
            print(f"{vq} {name}: {low} of {margin.numel()} frames with margin <= {MARGIN} (min {float(margin.min()):.3g}), "
                  f"{len(set(acts['idx'].reshape(-1).tolist()))} codes in use")
            assert low <= MARGIN_CAP * margin.numel(), "too many near-tie frames for an index fixture"
            fx[f"{vq}/{name}/idx"] = acts["idx"].reshape(B, -1).numpy()
            fx[f"{vq}/{name}/margin"] = margin.numpy()
            if name == "harm01_80000":
                fx[f"{vq}/{name}/bn_sub"] = bn[:, ::8, :].numpy()
        convert_fixture(net, os.path.join(GOLD, f"fx_e2e_{vq}.npz"))

    if want("keys_w2v2") or want("w2v2"):
        import torchaudio
        from oracle import wav2vec2 as ow
        torchaudio.models.wav2vec2.model._factory = ow.build_wav2vec2
        name2 = "bn_tdnnf_wav2vec2_100h_aug"
        net2, _ = reference_net(ref, name2)
        json.dump(keys_of(net2.bn_extractor), open(os.path.join(GOLD, "state_dict_keys_w2v2_novq.json"), "w"))
        assert not any("bottleneck_func" in k for k in net2.bn_extractor.state_dict())
        if want("w2v2"):
            with torch.no_grad():
                fx[f"{name2}/harm01_16000/bn"] = net2.get_bn(synthetic.harm_batch([0, 1], 16000)).numpy()

    np.savez_compressed(fx_path, **fx)
    assert os.path.getsize(fx_path) <= 1058046
    print("fixtures written to", GOLD, {k: v.shape for k, v in fx.items()})


if __name__ == "__main__":
    main()
