"""Host side of the ragged batches of the ResNet x-vector extractor (csrc/ragged2d/, include/satools_hip_ragged2d.h), CPU only: the tables
of the four time resolutions (ops.ragged_levels / ragged_column_segments), the conditions on the bounds rows and shapes of
tests/test_hip_xvector_resnet_ragged.py (header, binding and table are held together by tests/test_components_host.py), and
extract_batch's argument checks, which come before any device call."""
import os
import re

import numpy as np
import pytest
import torch

import test_hip_xvector_resnet_ragged as hr
from satools_amd import _lib, ops, xvector_resnet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "satools_hip_ragged2d.h"


# ---- the tables ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frames", [(9,), (9, 10, 16, 17, 63, 64, 65, 151), (501, 9, 1201, 33), tuple(range(9, 60)), (70000, 9)])
def test_ragged_levels_follow_the_nets_recurrence_and_the_layout_rule(frames):
    levels = ops.ragged_levels(frames)
    assert len(levels) == ops.RESNET_LEVELS == 4
    want = list(frames)
    for l, (off, length, t_tot) in enumerate(levels):
        assert off.dtype == length.dtype == np.int32 and length.tolist() == want, l
        o2, n2, t2 = ops.ragged_layout(want)                                      # every level by the existing rule, on its own
        assert off.tolist() == o2.tolist() and t_tot == t2
        want = [(t - 1) // 2 + 1 for t in want]                                   # T_{l+1} = (T_l - 1) // 2 + 1
    assert levels[3][1].tolist() == [xvector_resnet.pooled_frames(t) for t in frames]
    text = open(os.path.join(ROOT, "include", HEADER)).read()
    assert "T_i^{l+1} = (T_i^l - 1) / 2 + 1" in text


@pytest.mark.parametrize("frames", [(2,), (2, 3, 9, 2), (19, 2, 151)])
def test_the_column_index_names_each_segments_columns(frames):
    off, length, t_tot = ops.ragged_layout(frames)
    col = ops.ragged_column_segments(off, length, t_tot)
    assert col.dtype == np.int32 and col.shape == (t_tot,)
    for i, (o, n) in enumerate(zip(off, length)):
        assert (col[o:o + n] == i).all()
    assert col.min() >= 0 and col.max() == len(frames) - 1                        # a gap column names a valid row


def test_ragged_levels_refuse_what_ragged_layout_refuses():
    for bad in ([], [3, 0, 2], [5] * 1025):
        with pytest.raises(_lib.SatError):
            ops.ragged_levels(bad)


def test_ragged_levels_uploads_everything_in_one_copy(monkeypatch):
    """RaggedLevels on a stubbed ring: one upload holding the four tables, the sample counts and the column index; level 0 has what the
    front end's segment kernels read of a RaggedTable"""
    seen = []

    class Ring:
        def upload(self, words, device):
            seen.append(words.copy())
            return torch.from_numpy(words.copy())

    monkeypatch.setattr(ops, "_ragged_ring", Ring())
    n = [1280, 8000, 24123]
    lv = ops.RaggedLevels(torch.device("cpu"), n_samples=n)
    assert len(seen) == 1 and seen[0].dtype == np.int32
    host = ops.ragged_levels([1 + k // 160 for k in n])
    assert seen[0].size == 8 * 3 + 3 + host[3][2]
    for l in range(4):
        assert lv[l].seg_off.tolist() == host[l][0].tolist() and lv[l].seg_len.tolist() == host[l][1].tolist() and lv[l].T_tot == host[l][2]
        assert lv[l].B == 3 and lv[l].frames == host[l][1].tolist()
    assert lv[0].n_samples.tolist() == n and list(lv[0].n_samples_host) == n and lv[0].frames == [9, 51, 151]
    assert lv.columns.tolist() == ops.ragged_column_segments(*host[3]).tolist()
    x = torch.arange(2 * lv[3].T_tot).view(2, -1)
    assert lv[3].segment(x, 1).shape == (2, lv[3].frames[1])


# ---- extract_batch's argument checks ---------------------------------------------------------------------------------------------
def test_the_net_has_extract_batch_and_checks_its_arguments_before_any_device_call(monkeypatch):
    from satools_amd import synthetic
    Net = xvector_resnet.build()
    assert hasattr(Net(), "extract_batch")
    net = Net(num_speakers=10)
    net.load_state_dict(synthetic.xvector_resnet_state(0, 10), strict=True)
    assert callable(net.extract_batch) and callable(net.embed_segments)

    def no_library():
        raise AssertionError("the library was reached")

    monkeypatch.setattr(_lib, "lib", no_library)
    monkeypatch.setattr(ops, "lib", no_library)
    monkeypatch.setattr(net, "_prepare", lambda device: no_library())
    with pytest.raises(_lib.SatError, match="no CPU fallback"):
        net.extract_batch([torch.zeros(8000)])
    with pytest.raises(_lib.SatError, match="no CPU fallback"):
        net.extract_batch((torch.zeros(2, 8000), [8000, 700]))                    # (the device check comes before the lengths', as in xvector.Net)
    with pytest.raises(_lib.SatError, match="1-D"):
        net.extract_batch([torch.zeros(2, 8000)])
    with pytest.raises(_lib.SatError, match="lengths"):
        net.extract_batch((torch.zeros(2, 8000), [8000, 9000]))
    with pytest.raises(_lib.SatError, match="empty"):
        net.extract_batch([])
    # the checks past the device's, on meta tensors that claim to live there
    cuda = lambda n: _OnDevice(n)
    with pytest.raises(_lib.SatError, match="1025 utterances"):
        net.extract_batch([cuda(1300)] * 1025)
    with pytest.raises(_lib.SatError, match="utterance 1 of 1279 samples"):
        net.extract_batch([cuda(8000), cuda(1279), cuda(700)])
    with pytest.raises(_lib.SatError, match=r"2\^31 bytes"):
        net.extract_batch([cuda(160 * 2100)] * 100)


class _OnDevice(torch.Tensor):
    """a 1-D tensor without storage that reports the HIP device: extract_batch's checks read shapes and `is_cuda` only"""

    @staticmethod
    def __new__(cls, n):
        return torch.Tensor._make_subclass(cls, torch.empty(n, device="meta"))

    is_cuda = property(lambda self: True)


# ---- what is particular to this component (tests/test_components_host.py holds header, binding, library, build and bounds table together) ----
def test_ops_has_the_wrappers_of_the_ragged2d_entries():
    for name in ("ragged_levels", "RaggedLevels", "conv2d_segments", "plane_mean_segments", "se_scale_add_relu_segments", "row_mean_std_segments"):
        assert callable(getattr(ops, name)), name


def test_every_ragged2d_bounds_row_runs_with_and_without_a_broken_table():
    for r in hr.ROWS:
        assert r.shapes and any(s[-1] for s in r.shapes) and any(not s[-1] for s in r.shapes), r.name      # with and without the broken entry


def test_the_gpu_tests_shapes_are_the_ones_the_kernels_edges_need():
    tile = open(os.path.join(ROOT, "sa-toolkit_amd", "csrc", "conv2d_tile.h")).read()        # the tile body both forms call
    th, tw = (int(re.search(rf"constexpr int {n} = (\d+);", tile).group(1)) for n in ("C2_TH", "C2_TW"))
    assert '#include "../conv2d_tile_body.h"' in open(os.path.join(ROOT, "sa-toolkit_amd", "csrc", "ragged2d", "resnet_ragged.hip")).read()
    assert (th, tw) == (4, 32)
    assert sorted(hr.WIDTHS) == [1, 2, tw - 1, tw, tw + 1, 2 * tw - 1, 2 * tw, 2 * tw + 1, 3 * tw + 1] and list(hr.WIDTHS) != sorted(hr.WIDTHS)
    assert {hr.out_widths((w,), 2)[0] for w in (63, 64, 65)} == {tw, tw + 1}
    assert hr.H_CONV == th + 1 and (hr.H_CONV - 1) // 2 + 1 == 3 and set(hr.WIDTHS_256) <= set(hr.WIDTHS) and len(hr.WIDTHS_256) == 3
    assert set(hr.CONVS) == {(1, 32, 3, 1), (32, 32, 3, 1), (32, 64, 3, 2), (32, 64, 1, 2), (64, 64, 3, 1), (64, 128, 3, 2), (128, 256, 1, 2), (256, 256, 3, 1)}
    assert hr.EPILOGUES == ("none", "affine", "affine_relu")
    counts = {H * t for H, ts in hr.PLANES_T.items() for t in ts}
    assert {63, 64, 65, 128, 129} <= counts and set(hr.PLANES_T) == {1, 5, 10} and hr.CHANNELS == (5, 8)
    assert {1, 65} <= {t for ts in hr.PLANES_T.values() for t in ts} and all(t <= 65 or (H == 1 and t in (128, 129)) for H, ts in hr.PLANES_T.items() for t in ts)
    assert sorted(hr.STD_LENGTHS) == [2, 3, 63, 64, 65, 129]
    assert sorted(hr.NET_SAMPLES) == [1280, 8000, 10079, 10080, 16000, 24123]
