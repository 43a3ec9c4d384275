"""Host side of the ResNet x-vector extractor (egs/asv/voxceleb/local/tuning/resnet.py), CPU only: the reference's checkpoint format
loads, the parameter tree has the reference's keys and shapes, the new C entries are declared, exported and bound under ABI 8, and
the model refuses what it cannot do."""
import json
import os
import re

import pytest
import torch

from satools_amd import _lib
from test_codegen_invariants import code_objects  # noqa: F401  (the module-scoped fixture)
from test_codegen_xvector_resnet import test_resnet_kernels_have_no_scratch_and_no_spills as _codegen_check

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sat_conv2d_f32", "sat_se_scale_add_relu_f32", "sat_row_mean_std_f32")


def _keys():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "state_dict_keys_xvector_resnet.json")))


def test_reference_checkpoint_format_loads(tmp_path):
    import satools_amd
    from satools_amd import synthetic
    sd = synthetic.xvector_resnet_state(0, 10)
    ck = {"task_path": "/egs/asv/voxceleb", "base_model_path": "local/tuning/resnet.py", "base_model_params": {"num_speakers": 10},
          "base_model_args": {}, "base_model_state_dict": sd}
    torch.save(ck, tmp_path / "final.pt")
    m = satools_amd.load_model(str(tmp_path / "final.pt"))
    assert m.embedding_size == 256 and not m.training
    got = m.state_dict()
    assert all(torch.equal(got[k], v) for k, v in sd.items())


def test_state_dict_keys_and_shapes_are_the_references():
    from satools_amd import synthetic, xvector_resnet
    want = _keys()
    net = xvector_resnet.build()(num_speakers=10)
    got = {k: list(v.shape) for k, v in net.state_dict().items()}
    assert got == want
    assert list(got) == list(want)                                     # the reference's order too
    net.load_state_dict(synthetic.xvector_resnet_state(0, 10), strict=True)
    assert want["after_speaker_embedding.weight"] == [10, 256] and want["stat_pooling.attention.0.weight"] == [128, 7680, 1]
    assert want["before_speaker_embedding.lin_be.weight"] == [256, 5120]
    # a shortcut in the first block of EVERY layer (the reference's tuple stride makes `stride != 1` true for layer1 too), nowhere else
    sc = sorted(k for k in want if k.endswith("shortcut.0.weight"))
    assert sc == [f"sequence_network.layer{i}.0.shortcut.0.weight" for i in (1, 2, 3, 4)]
    assert want[sc[0]] == [32, 32, 1, 1] and want[sc[3]] == [256, 128, 1, 1]
    convs = [k for k, v in want.items() if len(v) == 4]
    assert len(convs) == 37 and sum(1 for k in convs if want[k][2] == 3) == 33


def test_synthetic_state_sets_every_batchnorm_weight_by_module_type():
    from satools_amd import synthetic
    sd = synthetic.xvector_resnet_state(3, 10)
    for k in ("sequence_network.layer2.0.shortcut.1.weight", "stat_pooling.attention.2.weight", "sequence_network.bn1.weight",
              "before_speaker_embedding.bn_be.weight"):
        assert float(sd[k].min()) >= 0.8 and float(sd[k].max()) <= 1.2, k
    assert not torch.equal(sd["sequence_network.conv1.weight"], synthetic.xvector_resnet_state(4, 10)["sequence_network.conv1.weight"])


def test_synthetic_spec_builds():
    import satools_amd
    m = satools_amd.load_model("synthetic:xvector_resnet?speakers=12")
    assert tuple(m.after_speaker_embedding.weight.shape) == (12, 256)
    m2 = satools_amd.load_model("synthetic:xvector_resnet?seed=1&speakers=12")
    assert not torch.equal(m.sequence_network.conv1.weight, m2.sequence_network.conv1.weight)


def test_new_entries_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "satools_hip.h")).read()
    assert int(re.search(r"#define SAT_ABI_VERSION (\d+)", header).group(1)) == 8       # additive: no new ABI number
    lib = _lib.lib()
    for name in NEW:
        assert re.search(r"\bint " + name + r"\(", header), name
        assert hasattr(lib, name), name
        assert name in _lib.symbols("core")
    for name in re.findall(r"\b(sat_\w+)\(", header):                              # every declared entry is exported
        assert hasattr(lib, name), name
    from satools_amd import ops
    for fn in ("conv2d", "pack_conv2d_weight", "se_scale_add_relu", "row_mean_std"):
        assert callable(getattr(ops, fn))
    src = open(os.path.join(ROOT, "sa-toolkit_amd", "ops.py")).read()
    assert "ResNet x-vector extractor" in src


def test_codegen_of_the_new_kernels(code_objects):  # noqa: F811
    _codegen_check(code_objects)


def test_pack_conv2d_weight_layout():
    from satools_amd import ops
    w = torch.arange(2 * 3 * 3 * 3, dtype=torch.float32).reshape(2, 3, 3, 3)
    p = ops.pack_conv2d_weight(w)
    assert p.shape == (9, 3, 2) and float(p[1 * 3 + 2, 1, 0]) == float(w[0, 1, 1, 2])
    pt = ops.pack_conv2d_weight(w, transpose=True)
    assert float(pt[1 * 3 + 2, 1, 0]) == float(w[0, 1, 2, 1])
    with pytest.raises(_lib.SatError):
        ops.pack_conv2d_weight(torch.zeros(2, 3, 3))


def test_cpu_input_and_training_are_refused():
    import satools_amd
    m = satools_amd.load_model("synthetic:xvector_resnet")
    with pytest.raises(_lib.SatError):
        m(torch.zeros(16000))
    with pytest.raises(_lib.SatError):
        m.train()
    with pytest.raises(_lib.SatError):
        from satools_amd import ops
        ops.conv2d(torch.zeros(1, 32, 4, 4), torch.zeros(9, 32, 32), 3)
    from satools_amd import xvector_resnet
    assert xvector_resnet.pooled_frames(8) == 1 and xvector_resnet.pooled_frames(9) == 2
