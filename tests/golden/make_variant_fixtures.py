#!/usr/bin/env python3
"""Golden fixtures of the reference's two other anonymizer configs, local/tuning/hifigan_clean.py (per-speaker F0 statistics) and
local/tuning/hifigan_m2o.py (many-to-one), made by IMPORTING THE REFERENCE in the build container like make_fixtures.py (whose helpers
this script uses).  Run from the repo root:   python tests/golden/make_variant_fixtures.py

The nets are built through the reference's own `build(args)` of both files, on the fbank VQ extractor (bn_tdnnf_600h_vq_48) and on one
without a quantiser (bn_tdnnf_600h_aug), and loaded strictly with the synthetic state dicts of `synthetic:clean_hifigan_<asrbn>` /
`synthetic:hifigan_m2o_<asrbn>`.  Data only is written:
  state_dict_keys_hifigan_clean.json, state_dict_keys_hifigan_m2o.json     key / shape / dtype lists of the reference nets
  fx_variants.npz, per case <config>/<asrbn>/<case>/...
      wav            the waveforms (0.6 - 1 s)                     targets     indices into net.spk (clean)
      f0             the track handed over (the reference's torch YAAPT of the batch, [B, T'])
      f0_after       what the reference left in the caller's tensor: the normalised values
      y              convert()'s output
      x_bn_last, x_f0, x_spk     the generator's input: its last bn channel, its F0 row, every speaker row (clean)
      x_sums         float64 sums of every channel of the generator's input (the rest, as checksums)
    and clean/buffer (the SpeakerCMVN buffer as the reference serialised it, trailing zeros trimmed), clean/table ([n_spk, 2] = the
    mean / std it deserialised to), clean/missing_* (the exception of a target without statistics).
Cases: B = 1; B = 2 with two different targets (clean normalises the whole batch with the FIRST target's statistics); quant_16_awgn_2 under
torch.manual_seed(1234); m2o with a set_f0 that has no effect; clean with a target whose statistics are missing."""
import json
import os

import numpy as np

from make_fixtures import F0_OPTS, GOLD, exec_config, setup_reference

VQ, AUG = "bn_tdnnf_600h_vq_48", "bn_tdnnf_600h_aug"
CONFIG = {"clean": "hifigan_clean.py", "m2o": "hifigan_m2o.py"}
TAG = {"clean": "clean_hifigan_{}_v1", "m2o": "hifigan_m2o_{}_v1"}
SEED_AWGN = 1234
MISSING = 5          # index of the speaker whose statistics the missing-statistics case leaves out


def reference_net(ref, kind, asr_name, f0_transformation=""):
    import satools
    import torch
    from satools_amd import infer_helper, synthetic
    conf = dict(infer_helper.asrbn_conf_from_name(synthetic.ASR_DIR.format(name=asr_name)))
    conf["install_path"] = ref
    d = f"{ref}/egs/asr/librispeech/exp/chain/{asr_name}"
    os.makedirs(d, exist_ok=True)
    torch.save(conf, f"{d}/conf.pt")
    cfg = exec_config(f"{ref}/egs/vc/libritts/local/tuning/{CONFIG[kind]}")
    args = satools.utils.SimpleNamespace(asrbn_model=synthetic.ASR_DIR.format(name=asr_name), f0_transformation=f0_transformation)
    net = cfg.build(args)(utt2spk=synthetic.utt2spk())
    state, mine = synthetic.checkpoint(TAG[kind].format(asr_name))
    # (before the load: the reference's SpeakerCMVN.state_dict() serialises its CURRENT attributes over the buffer, loaded or not)
    assert list(net.state_dict()) == list(mine.state_dict()), "key order differs from the reference's"
    res = net.load_state_dict(state["base_model_state_dict"], strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    net.eval()
    return net, state


def run_case(net, fx, prefix, wav, targets=None, set_f0=None, seed=None):
    """one convert() with the generator's input captured; `set_f0`: "track" hands the reference's own track over, a tensor hands THAT over"""
    import torch
    from satools.hifigan import yaapt as ref_yaapt
    seen = {}
    h = net.hifigan.register_forward_pre_hook(lambda m, a: seen.update(x=a[0].detach().clone()))
    track = ref_yaapt.yaapt(wav.clone(), F0_OPTS)                    # [B, T']
    handed = None
    if set_f0 is not None:
        handed = (track if isinstance(set_f0, str) else set_f0).clone()
        fx[prefix + "f0"] = handed.numpy().copy()
        net.set_f0(handed)
    if seed is not None:
        torch.manual_seed(seed)
    with torch.no_grad():
        y = net.convert(wav.clone(), target=[net.spk[t] for t in targets]) if targets is not None else net.convert(wav.clone())
    h.remove()
    x = seen["x"]
    c_bn = 256
    fx[prefix + "wav"] = wav.numpy()
    fx[prefix + "track"] = track.numpy()
    if targets is not None:
        fx[prefix + "targets"] = np.asarray(targets, dtype=np.int64)
    if handed is not None:
        fx[prefix + "f0_after"] = handed.numpy().copy()
    fx[prefix + "y"] = y.numpy()
    fx[prefix + "x_bn_last"] = x[:, c_bn - 1].numpy()
    fx[prefix + "x_f0"] = x[:, c_bn].numpy()
    if x.shape[1] > c_bn + 1:
        fx[prefix + "x_spk"] = x[:, c_bn + 1:].numpy().astype(np.uint8)          # one-hot rows: 0 / 1
        assert np.array_equal(fx[prefix + "x_spk"].astype(np.float32), x[:, c_bn + 1:].numpy())
    fx[prefix + "x_sums"] = x.double().sum(dim=2).numpy()
    print(prefix, "x", tuple(x.shape), "y", tuple(y.shape))
    return x, y


def main():
    ref = setup_reference()
    import torch
    torch.set_num_threads(1)          # the reference's own YAAPT setting
    import satools  # noqa: F401  (the reference)
    from satools_amd import synthetic
    fx = {}
    w1 = synthetic.harm_batch([0], 16000)
    w2 = synthetic.harm_batch([0, 1], 9600)
    w3 = synthetic.harm_batch([2], 9600)

    # ---- clean ------------------------------------------------------------------------------------------------------------------------------
    net, state = reference_net(ref, "clean", VQ)
    run_case(net, fx, f"clean/{VQ}/b1/", w1, targets=[3], set_f0="track")
    x, _ = run_case(net, fx, f"clean/{VQ}/b2_two_targets/", w2, targets=[3, 10], set_f0="track")
    assert x.shape[1] == 256 + 1 + len(net.spk)
    # (the reference has deserialised its buffer by now: what state_dict() writes is its own serialisation)
    json.dump([[k, list(v.shape), str(v.dtype)] for k, v in net.state_dict().items()], open(os.path.join(GOLD, "state_dict_keys_hifigan_clean.json"), "w"))
    buf = net.state_dict()["f0_norm.model_state_buffer"].numpy()
    fx["clean/buffer"] = np.trim_zeros(buf, "b")
    st = net.f0_norm.speaker_stats
    fx["clean/table"] = np.asarray([[float(st[str(i)]["mean"]), float(st[str(i)]["std"])] for i in range(len(net.spk))], dtype=np.float32)
    assert all(st[str(i)]["mean"].dtype == torch.float32 for i in range(len(net.spk)))
    netq, _ = reference_net(ref, "clean", VQ, f0_transformation="quant_16_awgn_2")
    run_case(netq, fx, f"clean/{VQ}/quant_16_awgn_2/", w3, targets=[7], set_f0="track", seed=SEED_AWGN)
    neta, _ = reference_net(ref, "clean", AUG)
    run_case(neta, fx, f"clean/{AUG}/b2_two_targets/", w2, targets=[10, 3], set_f0="track")
    # a target without statistics
    netm, statem = reference_net(ref, "clean", VQ)
    sd = dict(statem["base_model_state_dict"])
    sd["f0_norm.model_state_buffer"] = synthetic.speaker_cmvn_buffer(len(netm.spk), 0, skip=(MISSING,))
    netm.load_state_dict(sd, strict=True)
    from satools.hifigan import yaapt as ref_yaapt
    netm.set_f0(ref_yaapt.yaapt(w3.clone(), F0_OPTS))
    try:
        with torch.no_grad():
            netm.convert(w3.clone(), target=[netm.spk[MISSING]])
        raise AssertionError("the reference did not raise")
    except RuntimeError as e:
        fx["clean/missing_type"] = np.asarray(type(e).__name__)
        fx["clean/missing_message"] = np.asarray(str(e))
        fx["clean/missing_speaker"] = np.asarray(MISSING)
        print("missing statistics:", type(e).__name__, e)

    # ---- m2o --------------------------------------------------------------------------------------------------------------------------------
    net, state = reference_net(ref, "m2o", VQ)
    json.dump([[k, list(v.shape), str(v.dtype)] for k, v in net.state_dict().items()], open(os.path.join(GOLD, "state_dict_keys_hifigan_m2o.json"), "w"))
    assert not hasattr(net, "spk")
    x, y = run_case(net, fx, f"m2o/{VQ}/b1/", w1)
    assert x.shape[1] == 257
    # a track handed over by set_f0 is never read: the output is that of the plain call, the handed tensor stays as it was
    bogus = torch.full((2, 31), 123.0)
    xa, ya = run_case(net, fx, f"m2o/{VQ}/b2_set_f0_ignored/", w2, set_f0=bogus)
    net.f0 = None
    xb, yb = run_case(net, {}, "scratch/", w2)
    assert torch.equal(ya, yb) and torch.equal(xa, xb) and bool((fx[f"m2o/{VQ}/b2_set_f0_ignored/f0_after"] == 123.0).all())
    netq, _ = reference_net(ref, "m2o", VQ, f0_transformation="quant_16_awgn_2")
    run_case(netq, fx, f"m2o/{VQ}/quant_16_awgn_2/", w3, seed=SEED_AWGN)
    neta, _ = reference_net(ref, "m2o", AUG)
    run_case(neta, fx, f"m2o/{AUG}/b1/", w3)

    path = os.path.join(GOLD, "fx_variants.npz")
    np.savez_compressed(path, **fx)
    print("written", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) <= 1 << 20, "larger than a committed file may be"


if __name__ == "__main__":
    main()
