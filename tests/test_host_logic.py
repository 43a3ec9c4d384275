"""Host-side logic, CPU only (no GPU compute calls); the C-ABI surface is held by tests/test_components_host.py."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import satools_amd
from satools_amd import _lib, f0, f0_transforms, infer_helper, packing, synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_hip_calls_fail_loudly_without_a_device_tensor():
    with pytest.raises(_lib.SatError):
        _lib.ptr(torch.zeros(4))
    model = satools_amd.load_model("synthetic:hifigan_bn_tdnnf_600h_vq_48_v1")
    with pytest.raises(_lib.SatError):
        model.get_bn(torch.zeros(1, 8000))            # model on the CPU: no fallback


def test_state_dict_keys_match_the_reference(gold, fbank_tag_state):
    state, net = fbank_tag_state
    ref = gold.json("state_dict_keys_fbank.json")
    mine = [[k, list(v.shape), str(v.dtype)] for k, v in net.state_dict().items()]
    assert mine == ref
    # a reference-format checkpoint round-trips, and remove_weight_norm keeps the folded weights
    net.load_state_dict(state["base_model_state_dict"])
    w = net.hifigan.ups[0].folded_weight().clone()
    net.remove_weight_norm()
    assert "hifigan.ups.0.weight" in net.state_dict() and "hifigan.ups.0.weight_v" not in net.state_dict()
    assert torch.equal(net.hifigan.ups[0].folded_weight(), w)


def test_speaker_ids_are_bit_exact(gold):
    fx = gold.json("fx_spk.json")
    net = satools_amd.load_model("synthetic:hifigan_bn_tdnnf_600h_vq_48_v1")
    assert net.spk == fx["spk"]                       # Python string sort order ('1000' < '101' < '99')
    one = net.get_spk_id(torch.zeros(1, 400), fx["str_target"])
    assert list(one.shape) == fx["shape_str"] and str(one.dtype) == fx["dtype"]
    assert int(one.argmax()) == fx["str_onehot_argmax"] and int(one.sum()) == 1
    many = net.get_spk_id(torch.zeros(3, 400), fx["list_target"])
    assert many.argmax(1).tolist() == fx["list_onehot_argmax"]
    with pytest.raises(ValueError):
        net.get_spk_id(torch.zeros(1, 400), "unknown")


def test_load_model_resolution_and_errors(tmp_path):
    with pytest.raises(RuntimeError):
        satools_amd.load_model("https://github.com/deep-privacy/SA-toolkit/releases/download/x/final.pt")
    with pytest.raises(FileNotFoundError):
        satools_amd.load_model(str(tmp_path / "nope" / "final.pt"))
    state, _ = synthetic.checkpoint("bn_tdnnf_600h_vq_48_v1")
    p = tmp_path / "bn_tdnnf_600h_vq_48_v1"
    p.mkdir()
    torch.save(state, p / "final.pt")
    m = satools_amd.load_model(str(p / "final.pt"))
    assert m.padding == 19 and m.padding_after == 4   # get_padding(chain/model.py:466-473) // 2
    state["base_model_path"] = "local/chain/tuning/tdnnf_dp.py"
    torch.save(state, p / "final.pt")
    with pytest.raises(NotImplementedError):
        satools_amd.load_model(str(p / "final.pt"))
    conf = infer_helper.asrbn_conf_from_name("../../asr/librispeech/exp/chain/bn_tdnnf_wav2vec2_vq_48/final.pt")
    assert conf["base_model_path"].endswith("tdnnf_wav2vec2_vq.py") and conf["base_model_args"]["codebook_size"] == 48


def test_hub_tag_grammar(monkeypatch):
    import importlib.util
    spec = importlib.util.spec_from_file_location("hubconf", os.path.join(ROOT, "hubconf.py"))
    hub = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(hub)
    seen = {}
    monkeypatch.setattr(satools_amd, "load_model", lambda f, option_args=None: seen.update(f=f, o=option_args) or "m")
    assert hub._load("synthetic:hifigan_bn_tdnnf_600h_vq_48_v1+f0-transformation=quant_16_awgn_2") == "m"
    assert seen == {"f": "synthetic:hifigan_bn_tdnnf_600h_vq_48_v1", "o": {"f0_transformation": "quant_16_awgn_2"}}
    assert f0_transforms.parse_quant_bins("quant_16_awgn_2") == 16 and f0_transforms.parse_awgn_db("quant_16_awgn_2") == 2


def test_packing_layout_and_polyphase_equivalence():
    cin_pad, co_pad = packing.packed_dims(504, 512)
    assert (cin_pad, co_pad) == (512, 512)
    assert packing.packed_dims(16, 16) == (16, 64)
    w = torch.randn(20, 12, 3)
    p = packing.pack_conv_weight(w)
    assert p.shape == (1, 16, 3, 64)
    assert torch.equal(p[0, :12, :, :20], w.permute(1, 2, 0)) and not p[0, 12:].any() and not p[0, :, :, 20:].any()
    # ConvTranspose1d == conv with `u` output phases (the arithmetic the kernel relies on), on the CPU
    for k, u in ((11, 5), (8, 4), (4, 2), (16, 8)):
        x, wt = torch.randn(2, 6, 37), torch.randn(6, 5, k)
        ref = F.conv_transpose1d(x, wt, stride=u, padding=(k - u) // 2)
        wc, kp, pl = packing.convtranspose_as_phase_conv(wt, u, (k - u) // 2)
        y = F.conv1d(F.pad(x, (pl, kp - 1 - pl)), wc)              # [2, 5*u, 37], row co*u + r
        y = y.view(2, 5, u, 37).permute(0, 1, 3, 2).reshape(2, 5, 37 * u)
        assert torch.allclose(y, ref, atol=1e-5)


def test_grouped_polyphase_rows_and_their_zero_tap_mask():
    """sat_conv1d_desc.up_grouped / up_zero_taps (host side): the row order (16-channel group, phase, channel) is a permutation of
    the (channel, phase) order, the mask names exactly the all-zero (tap slot, phase) pairs of ConvTranspose1d(k, stride u, padding)
    seen as a polyphase conv (reference hifigan/archi.py:47-59), and the rule that admits a layer is the launcher's"""
    for k, u in ((8, 4), (4, 2), (16, 4), (6, 3)):
        pad = (k - u) // 2
        wt = torch.randn(8, 32, k)
        wc, kp, pl = packing.convtranspose_as_phase_conv(wt, u, pad)
        wg, kp2, pl2 = packing.convtranspose_as_phase_conv(wt, u, pad, grouped=True)
        assert (kp, pl) == (kp2, pl2) and wg.shape == wc.shape
        for c in (0, 5, 17, 31):
            for r in range(u):
                assert torch.equal(wg[(c // 16 * u + r) * 16 + c % 16], wc[c * u + r])
        mask = packing.convtranspose_zero_taps(k, u, pad)
        if kp <= 8:
            for slot in range(kp):
                for r in range(u):
                    assert bool((wc[r::u, :, slot] == 0).all()) == bool(mask >> (slot * 4 + r) & 1), (k, u, slot, r)
    assert packing.convtranspose_zero_taps(8, 4, 2) == 0x30c and packing.convtranspose_zero_taps(11, 5, 3) == 0        # (stride 5: no 4-bit phase field)
    # the mask is a promise about the weights, so it is RECORDED from them at pack time and a descriptor may only claim recorded zeros
    # (round-4 advisor item: a caller's mask used to be trusted)
    wg, kp, pl = packing.convtranspose_as_phase_conv(torch.randn(256, 128, 8), 4, 2, grouped=True)
    assert packing.grouped_zero_taps(wg, 4) == 0x30c
    wp = packing.pack_conv_weight_f16x3(wg, up=4)
    assert wp.up_zero_taps == 0x30c and packing.move_packed(wp, "cpu").up_zero_taps == 0x30c
    from satools_amd import ops
    x = torch.zeros(1, 256, 20)
    kw = dict(pad_left=pl, up=4, mode=1, up_grouped=True)
    ops._conv1d_desc(x, wp, 128, kp, up_zero_taps=0x30c, **kw)
    ops._conv1d_desc(x, wp, 128, kp, up_zero_taps=0x300, **kw)                  # fewer zeros claimed than there are: fine
    with pytest.raises(_lib.SatError):
        ops._conv1d_desc(x, wp, 128, kp, up_zero_taps=0x30d, **kw)              # slot 0 of phase 0 carries weights
    dense = packing.pack_conv_weight_f16x3(torch.randn(512, 256, 3), up=4)
    assert dense.up_zero_taps == 0
    with pytest.raises(_lib.SatError):
        ops._conv1d_desc(x, dense, 128, 3, up_zero_taps=0x30c, **kw)
    ok = packing.upsample_grouped_supported
    assert ok(256, 128, 8, 4, 2) and ok(128, 64, 8, 4, 2)
    assert not ok(512, 256, 11, 5, 3) and not ok(64, 32, 4, 2, 1) and not ok(64, 32, 8, 4, 2) and not ok(96, 64, 8, 4, 2) and not ok(128, 72, 8, 4, 2)


def test_yaapt_plan_matches_the_oracle_plan():
    from oracle import yaapt as oy
    opts = {"frame_length": 35.0, "frame_space": 20.0, "nccf_thresh1": 0.25, "tda_frame_length": 25.0}
    for n in (8000, 16384, 77040, 80000):
        P, Q = f0.make_plan(n, opts), oy.Plan(n, opts)
        for a, b in (("pad", "pad"), ("L", "L"), ("nframes", "nframes"), ("nl_lo", "nl_lo"), ("nl_hi", "nl_hi"),
                     ("wl", "wl"), ("half_wl", "half_wl"), ("min_shc", "min_shc"), ("max_shc", "max_shc"),
                     ("pk_center", "pk_center"), ("pk_min_lag", "pk_min_lag"), ("pk_max_lag", "pk_max_lag"),
                     ("tda_len", "tda_len"), ("tda_nframes", "tda_nframes"), ("nccf_center", "nccf_center")):
            assert getattr(P, a) == getattr(Q, b), (n, a)
    from oracle import biquad
    P = f0.make_plan(8000, opts)
    assert np.allclose(list(P.lp), [float(v) for v in biquad.kernel_constants("lp", 16000, 50.0)], rtol=0, atol=0)
    assert np.allclose(list(P.hp), [float(v) for v in biquad.kernel_constants("hp", 16000, 1500.0)], rtol=0, atol=0)


def test_yaapt_plan_matches_the_oracle_plan_under_every_option_set():
    """f0.make_plan against oracle.yaapt.Plan, field by field, for every option set of tests/yaapt_cases.py (the refused ones too:
    the plan is what the entry point refuses) and for the `frame_lengtht` spelling; `length_dims` against a full plan; and
    make_plan's own refusal, where the reference fails on a negative zero extension whatever the signal"""
    import yaapt_cases as yc
    from oracle import biquad
    from oracle import yaapt as oy
    ints = ("pad", "L", "nfft", "frame_size", "frame_jump", "nframes", "nl_lo", "nl_hi", "nframe_size", "half_wl", "wl", "max_shc", "min_shc",
            "nharm", "maxpeaks", "pk_center", "pk_min_lag", "pk_max_lag", "tda_len", "tda_nframes", "maxcands", "nccf_center", "median_value")
    scalars = ("nlfer_thresh1", "nlfer_thresh2", "shc_thresh1", "shc_thresh2", "f0_double", "f0_half", "merit_extra", "dp5_k1", "f0_min", "f0_max",
               "spec_pitch_min_std", "nccf_thresh1", "nccf_thresh2", "merit_pivot", "dp_w1", "dp_w2", "dp_w3", "dp_w4")
    sets = [(s.name, s.opts, [c.n for c in s.cases]) for s in yc.OPTION_SETS]
    sets.append(("frame_lengtht", {"frame_lengtht": 22.0, "frame_space": 15.0}, [20480]))
    sets.append(("both spellings", {"frame_lengtht": 22.0, "tda_frame_length": 24.0, "frame_space": 18.0}, [20480]))
    for name, opts, lengths in sets:
        for n in lengths + [lengths[0] + 1, lengths[0] // 2 + 3]:
            Q = oy.Plan(n, opts)
            P = f0._derive_plan(n, dict(opts))          # make_plan without its own refusal (below)
            for k in ints:
                assert getattr(P, k) == getattr(Q, k), (name, n, k, getattr(P, k), getattr(Q, k))
            for k in scalars:
                assert getattr(P, k) == np.float32(Q.p[k]), (name, n, k)
            assert (P.n, P.fs, P.delta, P.Lz) == (n, np.float32(Q.fs), np.float32(Q.delta), max(Q.L, Q.need)), (name, n)
            assert P.inv_shc_thresh1 == np.float32(1 / Q.p["shc_thresh1"]) and P.merit_boost1 == np.float32(1 + Q.p["merit_boost"])
            assert list(P.lp) == [float(v) for v in biquad.kernel_constants("lp", int(Q.fs), Q.p["bp_low"])], name
            assert list(P.hp) == [float(v) for v in biquad.kernel_constants("hp", int(Q.fs), Q.p["bp_high"])], name
            big = f0._derive_plan(3 * n, dict(opts))
            assert f0.length_dims(big, n) == [P.n, P.L, P.nframes, P.tda_nframes], (name, n)
            if Q.need < Q.L:
                with pytest.raises(_lib.SatError, match="frame_space too long for frame_length"):
                    f0.make_plan(n, dict(opts))
            else:
                assert bytes(f0.make_plan(n, dict(opts))) == bytes(P)
    assert oy.Plan(20480, {"frame_lengtht": 22.0}).tda_len == 352 and oy.Plan(20480, {"frame_lengtht": 22.0, "tda_frame_length": 24.0}).tda_len == 384
    s = yc.option_set("space_gt_frame")
    assert oy.Plan(s.cases[0].n, s.opts).need < oy.Plan(s.cases[0].n, s.opts).L


def test_fbank_tables_match_the_oracle():
    from oracle import fbank as ofb
    from satools_amd import asrbn
    assert torch.equal(asrbn.mel_banks(80), ofb.mel_banks(80).to(torch.float32))
    assert torch.equal(asrbn.povey_window(), ofb.povey_window())


def test_sharding_and_all_gather_two_ranks_gloo(tmp_path):
    """world_size 2 on the CPU (gloo): contiguous shards, fixed batches, one all-gather"""
    script = tmp_path / "w.py"
    script.write_text(f'''
import os, sys, torch, torch.distributed as dist
sys.path.insert(0, {ROOT!r})
import satools_amd
from satools_amd import dist as sdist
dist.init_process_group("gloo")
rank = dist.get_rank()
N = 11
calls = []
def conv(lo, hi):
    calls.append((lo, hi))
    return (torch.arange(lo, hi, dtype=torch.float32).view(-1, 1, 1) * torch.ones(1, 1, 5))
out = sdist.convert_sharded(conv, N, batch_size=4)
assert out.shape == (N, 1, 5) and torch.equal(out[:, 0, 0], torch.arange(N, dtype=torch.float32)), out[:, 0, 0]
exp = {{0: [(0, 4), (4, 6)], 1: [(6, 10), (10, 11)]}}[rank]
assert calls == exp, (rank, calls)
# a preallocated shard buffer filled by the callback (what bench.py does from its job streams) + the pre-gather hook
lo, hi = sdist.shard_bounds(N, rank, 2)
buf = torch.full((hi - lo, 1, 5), -1.0)
hooked = []
def fill(a, b):
    buf[a - lo:b - lo] = torch.arange(a, b, dtype=torch.float32).view(-1, 1, 1)
out2 = sdist.convert_sharded(fill, N, batch_size=4, local_out=buf, before_gather=lambda: hooked.append(1))
assert hooked == [1] and torch.equal(out2, out)
# the PCM16 gather (the int16 the reference writes, half the bytes): ragged shards, rows travel as bytes
out3 = sdist.convert_sharded(lambda a, b: (torch.arange(a, b, dtype=torch.float32).view(-1, 1, 1) / 32768.0) * torch.ones(1, 1, 5),
                             N, batch_size=4, transform=sdist.pcm16_rows)
assert out3.dtype == torch.int16 and out3.shape == (N, 1, 5) and torch.equal(out3[:, 0, 0], torch.arange(N, dtype=torch.int16)), out3[:, 0, 0]
assert torch.equal(sdist.pcm16_rows(torch.tensor([1.5, -1.5, 0.5 / 32768, 1.5 / 32768, -2.0])), torch.tensor([32767, -32768, 0, 2, -32768], dtype=torch.int16))
# the exchange issued in chunks of K batches while the shard is being filled (ChunkedGather): the result of the one-collective
# path — equal chunks go straight into their rows, the ragged last chunk (2 rows on rank 0, 1 on rank 1) travels padded
for K in (1, 2, 5):
    buf.fill_(-1.0)
    order, st = [], {{}}
    def before_chunk(c, a, b):
        order.append((c, a, b))
        assert bool((buf[a:b] >= 0).all())          # the chunk's batches have been produced when it is handed over
    out4 = sdist.convert_sharded(fill, N, batch_size=4, local_out=buf, gather_chunk_batches=K, before_chunk=before_chunk,
                                 before_gather=lambda: hooked.append(2), stats=st)
    assert torch.equal(out4, out), (K, out4[:, 0, 0])
    exp_chunks = {{1: [(0, 0, 4), (1, 4, hi - lo)], 2: [(0, 0, hi - lo)], 5: [(0, 0, hi - lo)]}}[K]
    assert order == exp_chunks, (K, order)
    assert len(st["chunks"]) == len(exp_chunks) and all("wait_ms" in c for c in st["chunks"])
# the chunks lag one chunk behind the launches (a batch's deferred work — rows that may be rewritten until its status has been checked —
# is never finished early for the collective); gather_chunk_lag=0 hands a chunk over right behind its last batch
for lag, exp_seen in ((1, [2, 2]), (0, [1, 2])):
    buf.fill_(-1.0)
    produced, seen = [0], []
    def fill_counting(a, b):
        produced[0] += 1
        fill(a, b)
    out7 = sdist.convert_sharded(fill_counting, N, batch_size=4, local_out=buf, gather_chunk_batches=1, gather_chunk_lag=lag,
                                 before_chunk=lambda c, a, b: seen.append(produced[0]))
    assert torch.equal(out7, out) and seen == exp_seen, (lag, seen)
out5 = sdist.convert_sharded(lambda a, b: buf.__setitem__(slice(a - lo, b - lo), (torch.arange(a, b, dtype=torch.float32).view(-1, 1, 1) / 32768.0) * torch.ones(1, 1, 5)),
                             N, batch_size=4, local_out=buf, transform=sdist.pcm16_rows, gather_chunk_batches=1)
assert out5.dtype == torch.int16 and torch.equal(out5, out3)
# equal shards (16 items): every chunk goes straight into its rows
lo16, hi16 = sdist.shard_bounds(16, rank, 2)
buf16 = torch.full((8, 1, 5), -1.0)
def fill16(a, b):
    buf16[a - lo16:b - lo16] = torch.arange(a, b, dtype=torch.float32).view(-1, 1, 1)
out6 = sdist.convert_sharded(fill16, 16, batch_size=4, local_out=buf16, gather_chunk_batches=1)
assert torch.equal(out6[:, 0, 0], torch.arange(16, dtype=torch.float32)) and out6.shape == (16, 1, 5)
# fewer items than ranks: refused on every rank before any collective (no hang)
try:
    sdist.convert_sharded(conv, 1, batch_size=4)
    raise SystemExit("expected ValueError")
except ValueError:
    pass
dist.barrier()
dist.destroy_process_group()
print("rank", rank, "ok")
''')
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
                        "--master-addr", "127.0.0.1", "--master-port", "29613", str(script)],
                       env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    from satools_amd import dist as sdist
    assert [sdist.shard_bounds(10, r, 3) for r in range(3)] == [(0, 4), (4, 7), (7, 10)]


def test_anonymize_config_parsing(tmp_path):
    """the reference's config file format ([cmd] / [<pipeline>] sections, ${:name} variables from [var] or the
    environment, satools/satools/bin/anonymize:22-79, script_utils.py:244-290)"""
    import configparser
    from satools_amd import anonymize as A
    cfg = configparser.ConfigParser()
    cfg.read_string("""
[var]
root = /data
[cmd]
device = cuda
ngpu = 0,2
jobs_per_compute_device = 2
pipeline = mypipe
[mypipe]
model = synthetic:hifigan_bn_tdnnf_600h_vq_48_v1
batch_size = 16
results_dir = ${:root}/wav
f0_modification =
target_selection_algorithm = constant
target_constant_spkid = 6081
""")
    s = A.vartoml(cfg)
    c = A.load_into(A.Cmd(), s["cmd"])
    p = A.load_into(A.Pipeline(), s[c.pipeline])
    assert c.ngpu == ["0", "2"] and c.jobs_per_compute_device == 2 and c.pipeline == "mypipe"
    assert p.batch_size == 16 and p.results_dir == "/data/wav" and p.f0_modification == "" and p.target_constant_spkid == "6081"
    assert p.data_loader_nj == 5 and p.new_datadir_suffix == "_anon"          # reference defaults
    os.environ["SAT_TEST_ROOT"] = "/env"
    try:
        cfg.read_string("[other]\nresults_dir = ${:SAT_TEST_ROOT}/x\n")
        assert A.vartoml(cfg)["other"]["results_dir"] == "/env/x"
    finally:
        del os.environ["SAT_TEST_ROOT"]


def test_remove_weight_norm_invalidates_the_packed_weight_key():
    """`remove_weight_norm()` (the reference Net API, hifigan.py:51-52) swaps weight_g / weight_v for a new
    `weight` Parameter; the generator's weight-cache key must follow the NEW tensors (no GPU needed for the key)"""
    from satools_amd.hifigan import CoreHifiGan
    g = CoreHifiGan(imput_dim=32, upsample_rates=[2, 2], upsample_kernel_sizes=[4, 4], upsample_initial_channel=32)
    for p in g.parameters():
        torch.nn.init.normal_(p, std=0.1)
    k0 = g._param_key()
    assert g._param_key() == k0
    w_before = g.conv_pre.folded_weight().clone()
    g.remove_weight_norm()
    k1 = g._param_key()
    assert k1 != k0 and g._packed_key is None
    assert "weight" in g.conv_pre._parameters and "weight_v" not in g.conv_pre._parameters
    assert torch.equal(g.conv_pre.folded_weight(), w_before)            # folding is exact
    with torch.no_grad():
        g.conv_post.weight.mul_(0.5)                                    # an in-place edit of the NEW parameter
    assert g._param_key() != k1
    sd = {k: v.clone() + 1 for k, v in g.state_dict().items()}
    g.load_state_dict(sd)
    assert g._param_key() != k1


def test_bench_gpus_2_as_typed_spawns_its_ranks(tmp_path):
    """`python bench.py --gpus 2` without torch.distributed.run around it: the parent starts the ranks as a child
    process and relays the JSON line and the exit code (dry run on the CPU: gloo, stand-in convert, the same
    convert_sharded call as the GPU path)"""
    env = dict(os.environ, SAT_BENCH_DRYRUN="1", MASTER_ADDR="127.0.0.1")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1"],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
    out = json.loads(line)
    assert out["n_gpus"] == 2 and out["steps"] == 3 and out["config"]["utterances"] == 2 * 3 * 32
    # a failing rank's exit code comes back through the parent
    env["SAT_BENCH_DRYRUN"] = "0"
    env["HIP_VISIBLE_DEVICES"] = ""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0


def test_conv_options_from_the_environment(monkeypatch):
    """SATOOLS_AMD_CONV_OPTIONS="name=value,..." is applied through sat_conv_set_option when the library is loaded
    (whole-program A/B runs, tools/ab_bench.sh); an unknown name fails loudly"""
    from satools_amd import _lib
    saved = _lib._lib
    try:
        _lib._lib = None
        monkeypatch.setenv("SATOOLS_AMD_CONV_OPTIONS", "pair32w=0, lean_balance=2")
        l = _lib.lib()
        assert l.sat_conv_set_option(b"pair32w", 1) == 0 and l.sat_conv_set_option(b"lean_balance", 1) == 0      # back to the defaults
        _lib._lib = None
        monkeypatch.setenv("SATOOLS_AMD_CONV_OPTIONS", "no_such_switch=1")
        with pytest.raises(_lib.SatError, match="no_such_switch"):
            _lib.lib()
    finally:
        _lib._lib = saved


def test_f16f8r_weight_packing_layout():
    """packing.pack_conv_weight_f16f8r (SAT_CONV_F16F8R, include/satools_hip.h): [2 ceil(C_in/32 K / 2) steps][8 planes][co_pad][16 B] over
    the LINEAR sequence of (channel pair, tap): E steps carry hi f16 (plane = 4 element + 2 chunk + half), O steps e4m3(lo 2^9) |
    e4m3(hi 2^-2) (plane = 4 element + 2 term + chunk); the layer scale of the SAT_CONV_F16X3 packing; pairs straddle channel pairs
    (an odd K costs nothing), only an odd total ends with a zero element"""
    torch.manual_seed(3)
    f8 = lambda t, ex: (t.float() * 2.0 ** ex).clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8)
    for cin, k in ((64, 7), (96, 3), (64, 4)):
        w = torch.randn(128, cin, k) * 0.05
        p = packing.pack_conv_weight_f16f8r(w)
        p3 = packing.pack_conv_weight_f16x3(w)
        nlin = cin // 32 * k
        nq = (nlin + 1) // 2
        assert p.shape == (2 * nq, 8, 128, 16) and p.dtype == torch.uint8 and p.w_descale == p3.w_descale
        e = packing.f16x3_scale_exponent(w)
        ws = w * 2.0 ** e
        assert 2 ** 9 <= float(ws.abs().max()) < 2 ** 10
        hi = ws.half()
        lo = (ws - hi.float()).half()
        for q in range(nq):
            for j in range(2):
                L = 2 * q + j
                pp, tap = divmod(L, k)
                for c in range(2):
                    ch = slice(32 * pp + 16 * c, 32 * pp + 16 * c + 16)
                    for hf in range(2):
                        got = p[2 * q, 4 * j + 2 * c + hf].contiguous().view(torch.float16)           # [co][8]
                        exp = hi[:, 32 * pp + 16 * c + 8 * hf: 32 * pp + 16 * c + 8 * hf + 8, tap] if L < nlin else torch.zeros(128, 8, dtype=torch.float16)
                        assert torch.equal(got, exp), (cin, k, q, j, c, hf)
                    for term, (src, ex) in enumerate(((lo, 9), (hi, -2))):
                        got = p[2 * q + 1, 4 * j + 2 * term + c]
                        exp = f8(src[:, ch, tap], ex) if L < nlin else torch.zeros(128, 16, dtype=torch.uint8)
                        assert torch.equal(got, exp), (cin, k, q, j, term, c)
    with pytest.raises(ValueError):
        packing.pack_conv_weight_f16f8r(torch.randn(64, 48, 3))


def test_gpu_count_without_the_hip_runtime(monkeypatch):
    """`ngpu = all` of the anonymize config is resolved in the PARENT of the per-GPU workers, which must not initialise HIP
    (round-4 review): from the visibility variables, else from sysfs"""
    from satools_amd import anonymize
    monkeypatch.setenv("HIP_VISIBLE_DEVICES", "2,5,7")
    assert anonymize.parse_ngpu("all") == ["0", "1", "2"]
    monkeypatch.delenv("HIP_VISIBLE_DEVICES")
    monkeypatch.setenv("ROCR_VISIBLE_DEVICES", "0")
    assert anonymize.parse_ngpu("all-force") == ["0"]
    monkeypatch.delenv("ROCR_VISIBLE_DEVICES")
    monkeypatch.delenv("CUDA_VISIBLE_DEVICES", raising=False)
    assert len(anonymize.parse_ngpu("all")) >= 1                  # sysfs (none here: at least one id)
    assert anonymize.parse_ngpu("[0, 3]") == ["0", "3"]
    import inspect
    assert "torch" not in inspect.getsource(anonymize.parse_ngpu) and "torch" not in inspect.getsource(anonymize.visible_gpu_count)


def test_gpu_count_only_counts_render_nodes_this_process_can_open(tmp_path):
    """sysfs lists every GPU of the machine; a container given only some /dev/dri/renderD* nodes must count those
    (round-5 advisor item): a fake KFD topology of one CPU node and three GPUs, two of whose render nodes exist"""
    from satools_amd import anonymize
    props = []
    for i, (simd, minor) in enumerate([(0, -1), (1024, 128), (1024, 129), (1024, 130)]):
        d = tmp_path / "nodes" / str(i)
        d.mkdir(parents=True)
        (d / "properties").write_text(f"cpu_cores_count 0\nsimd_count {simd}\ndrm_render_minor {minor}\n")
        props.append(str(d / "properties"))
    dri = tmp_path / "dri"
    dri.mkdir()
    (dri / "renderD128").write_text("")
    (dri / "renderD130").write_text("")
    assert anonymize._count_kfd_gpus(props, str(dri), []) == 2
    (dri / "renderD129").write_text("")
    assert anonymize._count_kfd_gpus(props, str(dri), []) == 3
    assert anonymize._count_kfd_gpus(props, str(tmp_path / "no_such_dir"), []) == 3      # no render directory at all: the topology decides
    assert anonymize._count_kfd_gpus([], str(dri), []) == 0


def test_near_tie_windows_cover_their_frames():
    """asrbn.tie_windows (the input windows of the VQ guard's second decision, round 6): for random spans of near-tie frames the
    common window length and the per-row starts are aligned to the stack's stride, stay inside the utterance, and the output
    frames a window yields contain the span — checked against the receptive field of the fbank-tag stack built on the CPU"""
    import random
    from satools_amd import asrbn
    net = asrbn.TdnnfVqNet(output_dim=8)
    S, W = net._stack_receptive_field()
    assert (S, W) == (2, 39)
    layers = net._stack_layers()
    rng = random.Random(3)
    for _ in range(2000):
        Tf = rng.randint(W, 1900)
        Tq = (Tf - W) // S + 1
        assert net._layers_out_len(layers, Tf) == Tq
        spans = []
        for _ in range(rng.randint(1, 4)):
            lo = rng.randint(0, Tq - 1)
            spans.append((lo, rng.randint(lo, min(Tq - 1, lo + rng.choice([0, 0, 1, 5, 40, 400])))))
        L, starts = asrbn.tie_windows(Tf, S, W, spans)
        assert W <= L <= Tf and (Tf - L) % S == 0
        Lq = net._layers_out_len(layers, L)
        assert Lq == (L - W) // S + 1
        for (lo, hi), a in zip(spans, starts):
            assert a % S == 0 and 0 <= a and a + L <= Tf
            t0 = a // S
            assert t0 <= lo and hi <= t0 + Lq - 1 and t0 + Lq <= Tq, (Tf, spans, L, starts)


def test_ragged_yaapt_length_dims_are_the_plans():
    """f0.length_dims(P, n) — what a ragged batch sends per utterance — equals the length-dependent fields of a full make_plan(n)"""
    from satools_amd import f0
    for opts in ({"frame_length": 35.0, "frame_space": 20.0, "nccf_thresh1": 0.25, "tda_frame_length": 25.0}, {}, {"frame_lengtht": 30.0, "frame_space": 5.0}):
        P = f0.make_plan(80000, dict(opts))
        for n in list(range(600, 1400)) + list(range(47990, 48330)) + [16000, 16001, 79999, 80000, 560001]:
            q = f0.make_plan(n, dict(opts))
            assert f0.length_dims(P, n) == [q.n, q.L, q.nframes, q.tda_nframes], (opts, n)
            assert (q.pad, q.frame_jump, q.frame_size, q.tda_len) == (P.pad, P.frame_jump, P.frame_size, P.tda_len)


def test_frozen_files_of_older_formats_are_refused(tmp_path):
    """a frozen file of format /2 (written before the near-tie guard's calibration and exact-f32 packings travelled with it) or /1
    is refused with the re-export message before anything is built, and a file of the current format is named"""
    from satools_amd import frozen
    assert frozen.FORMAT == "satools_amd.frozen/3"
    for old in ("satools_amd.frozen/2", "satools_amd.frozen/1"):
        path = str(tmp_path / (old[-1] + ".frozen"))
        torch.save({"format": old, "kind": "anonymizer", "extractor": {}}, path)
        with pytest.raises(_lib.SatError, match="re-export"):
            frozen.load_frozen(path, "cpu")
    path = str(tmp_path / "other.frozen")
    torch.save({"format": "something else"}, path)
    with pytest.raises(_lib.SatError, match="not a satools_amd.frozen/3"):
        frozen.load_frozen(path, "cpu")
