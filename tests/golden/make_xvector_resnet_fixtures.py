#!/usr/bin/env python3
"""Golden fixtures for the ResNet x-vector extractor: builds the REFERENCE's half-ResNet34 Net through its own model-config
`build(args)` (egs/asv/voxceleb/local/tuning/resnet.py), loads the seeded synthetic state dict of
satools_amd.synthetic.xvector_resnet_state strictly (pins key names and shapes), and stores its outputs on seeded synthetic
utterances: the x-vector, the pooled statistics, and strided samples of the stem's output and of every layer's, in the reference's
own [B, C, T, F] layout.  Next to every tensor goes `<name>_f32_dev`: the largest deviation, over the WHOLE tensor, of this float32
forward from the same Net's forward in float64 (`net.double()`): the yardstick the device tests scale their bars with.
torchaudio's MelSpectrogram is the stand-in of tests/golden/refstub.     python tests/golden/make_xvector_resnet_fixtures.py"""
import copy
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_fixtures as mf   # noqa: E402

#: sampling of the [1, C, T, F] layer outputs (channel, time, frequency steps)
SUB = (4, 3, 3)
UTTERANCES = (("harm0_16000", 0, 16000), ("harm3_48000", 3, 48000), ("harm7_24123", 7, 24123))
TAPS = ("bn1", "layer1", "layer2", "layer3", "layer4", "pooled")


def hooked(net):
    got = {}
    sn = net.sequence_network
    # the hook sees bn1's output; forward applies its ReLU outside the module, so it is applied here
    sn.bn1.register_forward_hook(lambda _m, _i, o: got.__setitem__("bn1", torch.relu(o.detach())))
    for name in ("layer1", "layer2", "layer3", "layer4"):
        getattr(sn, name).register_forward_hook(lambda _m, _i, o, name=name: got.__setitem__(name, o.detach().clone()))
    net.stat_pooling.register_forward_hook(lambda _m, _i, o: got.__setitem__("pooled", o.detach()))
    return got


def main():
    ref = mf.setup_reference()
    import satools_amd   # noqa: F401
    from satools_amd import synthetic
    m = mf.exec_config(os.path.join(ref, "egs/asv/voxceleb/local/tuning/resnet.py"))
    net = m.build(types.SimpleNamespace())(num_speakers=10)
    net.eval()
    print("strict load ok:", net.load_state_dict(synthetic.xvector_resnet_state(0, 10), strict=True))
    json.dump({k: list(v.shape) for k, v in net.state_dict().items()}, open(os.path.join(HERE, "state_dict_keys_xvector_resnet.json"), "w"), indent=0)
    net64 = copy.deepcopy(net).double()
    got, got64 = hooked(net), hooked(net64)
    out = {}
    for tag, seed, n in UTTERANCES:
        wav = synthetic.harm_batch([seed], n)[0]
        with torch.no_grad():
            xv = net(wav)[1]
            xv64 = net64(wav.double())[1]
        got["xvector"], got64["xvector"] = xv, xv64
        for name in TAPS + ("xvector",):
            a, b = got[name], got64[name]
            assert a.dtype == torch.float32 and b.dtype == torch.float64 and a.shape == b.shape, (name, a.dtype, b.dtype)
            out[f"{tag}/{name}_f32_dev"] = np.float64((a.double() - b).abs().max())
            keep = a[:, ::SUB[0], ::SUB[1], ::SUB[2]] if a.dim() == 4 else a
            out[f"{tag}/{name}"] = keep.contiguous().numpy()
            print(tag, name, tuple(a.shape), "->", tuple(keep.shape), "rms %.3f max %.2f f32_dev %.3e" % (
                float(a.pow(2).mean().sqrt()), float(a.abs().max()), float(out[f"{tag}/{name}_f32_dev"])))
    np.savez_compressed(os.path.join(HERE, "fx_xvector_resnet.npz"), **out)
    print("fx_xvector_resnet.npz:", os.path.getsize(os.path.join(HERE, "fx_xvector_resnet.npz")), "bytes")


if __name__ == "__main__":
    main()
