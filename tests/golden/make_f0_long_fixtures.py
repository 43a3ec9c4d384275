#!/usr/bin/env python3
"""The reference's own word on utterances BEYOND 2048 F0 frames (tests/yaapt_long_cases.py), made by IMPORTING THE REFERENCE in the build
container like make_f0_edge_fixtures.py (whose helpers this script uses).  Run from the repo root:
    python tests/golden/make_f0_long_fixtures.py [--only f0 fbank w2v2]

Data only is written:
  fx_f0_long.npz       <case name>         the F0 track [1, nframes] of the reference's `yaapt(wav, opts)`, float32
                       raised/<case name>  the exception's type name as a string, else ""  (every case)
  fx_convert_long.npz  the reference's own Net on ONE `harm` utterance of 655 361 samples (2049 frames: `_long_batch([3], n)` of
                       tests/test_hip_robust.py), for the fbank tag and the wav2vec2 tag, per tag under "<tag key>/":
                       f0             net.get_f0(w)                                  [1, 2049]
                       idx, d1, d2    the VQ indices and the two smallest distances of every frame, as in fx_w2v2_long.npz
                       convert_every16  every 16th sample of net.convert(w, target=net.spk[5])
                       and "seeds", "n" for the input
Each part of fx_convert_long.npz is made by its own --only word and merged into the file, so one tag can be redone alone."""
import argparse
import os
import sys

import numpy as np

from make_f0_edge_fixtures import builtin_name
from make_fixtures import F0_OPTS, GOLD, ROOT, build_reference_model, setup_reference

N_LONG = 655361
SEED = 3
TAGS = {"fbank": ("bn_tdnnf_600h_vq_48", 20), "w2v2": ("bn_tdnnf_wav2vec2_vq_48", 2)}        # ASR model of the tag, its VQ layer


def long_wav(n=N_LONG, seed=SEED):
    """tests/test_hip_robust.py: _long_batch([seed], n)"""
    import torch
    from satools_amd import synthetic
    seeds = [seed + 7 * j for j in range((n + 79999) // 80000)]
    return seeds, torch.cat([synthetic.harm_batch([s], 80000)[0] for s in seeds])[:n].unsqueeze(0)


def f0_part():
    from satools.hifigan import yaapt as ref_yaapt      # the reference (sets one thread)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import yaapt_long_cases as ylc
    assert ylc.OPTS == F0_OPTS
    out = {}
    for case in ylc.CASES:
        wav = case.wav().unsqueeze(0)
        try:
            track = ref_yaapt.yaapt(wav, dict(F0_OPTS))
            raised = ""
            out[case.name] = track.numpy().astype(np.float32)
            assert out[case.name].shape == (1, case.nframes), (case, out[case.name].shape)
        except Exception as e:                           # noqa: BLE001  (the type is the recorded result)
            raised = builtin_name(e)
        out["raised/" + case.name] = np.array(raised)
        want = case.raises or ""
        print(f"{case.name:28s} frames={case.nframes} raised={raised!r:16s} voiced frames={int((out[case.name] > 0).sum()) if not raised else '-'}"
              + ("" if raised == want else f"   !! the catalogue says {want!r}"), flush=True)
    np.savez_compressed(os.path.join(GOLD, "fx_f0_long.npz"), **out)
    print("wrote fx_f0_long.npz:", os.path.getsize(os.path.join(GOLD, "fx_f0_long.npz")), "bytes")


def convert_part(ref, key):
    import torch
    from satools_amd import synthetic
    name, vq_layer = TAGS[key]
    if key == "w2v2":
        import torchaudio
        from oracle import wav2vec2 as ow
        torchaudio.models.wav2vec2.model._factory = ow.build_wav2vec2
    net = build_reference_model(ref, name)
    st, _ = synthetic.checkpoint("hifigan_" + name + "_v1")
    net.load_state_dict(st["base_model_state_dict"], strict=True)
    net.eval()
    seeds, w = long_wav()
    acts = {}
    h = net.bn_extractor.tdnnfs[vq_layer].bottleneck_func.quant.register_forward_hook(lambda m, i, o: acts.update(idx=o[5].detach(), dist=o[4].detach()))
    out = {}
    with torch.no_grad():
        net.get_bn(w)
        out["idx"] = acts["idx"].reshape(1, -1).numpy()
        srt = acts["dist"].sort(1)[0]
        out["d1"] = srt[:, 0].reshape(1, -1).numpy()
        out["d2"] = srt[:, 1].reshape(1, -1).numpy()
        out["f0"] = net.get_f0(w).numpy()
        out["convert_every16"] = net.convert(w.clone(), target=net.spk[5]).numpy()[..., ::16]
    h.remove()
    path = os.path.join(GOLD, "fx_convert_long.npz")
    merged = dict(np.load(path)) if os.path.exists(path) else {}
    merged.update({f"{key}/{k}": v for k, v in out.items()})
    merged.update(seeds=np.array(seeds), n=np.array(N_LONG))
    np.savez_compressed(path, **merged)
    print(f"{key}:", {k: v.shape for k, v in out.items()}, "fx_convert_long.npz:", os.path.getsize(path), "bytes", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", nargs="*", default=None)
    a = ap.parse_args()
    want = lambda name: a.only is None or name in a.only
    ref = setup_reference()
    if want("f0"):
        f0_part()
    for key in TAGS:
        if want(key):
            convert_part(ref, key)


if __name__ == "__main__":
    main()
