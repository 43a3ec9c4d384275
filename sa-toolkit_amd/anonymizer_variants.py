"""The reference's two other anonymizer model configs behind the same interface as anonymizer.py:

  local/tuning/hifigan_clean.py   F0 normalised per TARGET speaker with stored statistics (SpeakerCMVN), otherwise hifigan.py
  local/tuning/hifigan_m2o.py     many-to-one: no target, no one-hot, `convert(x)`, 257 generator input channels

Both differ from hifigan.py only between the extractors and the generator, and both take that stretch as ONE launch
(ops.generator_input, include/satools_hip_geninput.h): the bottleneck features through the strides the extractor left them in, the raw
track normalised with a row of a statistics table, quantised / noised, resampled, the speaker rows broadcast.  The existing config's
path (anonymizer.py) is not touched; its class is subclassed here for everything the configs share.

Quirks kept from the reference:
  * clean: the statistics are keyed by the INDEX STRING of the target (get_one_hot_str_from_tensor), and each slice of dim 0 of the 3-D
    track is normalised with the statistics of spk_id[i].  In convert() the track is [1, B, T]: ONE slice, so the WHOLE batch is
    normalised with the FIRST target's statistics.
  * clean: a target without computed statistics raises the reference's RuntimeError (pass_though_if_not_computed is training-only).
  * clean: the state arrives as the pickled byte buffer `f0_norm.model_state_buffer` (900 000 uint8) and is deserialised once.
  * m2o: extract_features never reads a track handed over by set_f0 (set_f0 exists all the same); the net has no `spk`.
  * both: the normalised values are left in the caller's F0 tensor.
Deviation: the reference's clean config tracks F0 with the numpy `pyaapt` (another tracker: FIR band-pass, float64).  get_f0 here runs
the device YAAPT of the other configs; the batch job hands the track over with set_f0 either way.
Not built for these configs: convert_padded, frozen export (both refused by name), the training-only paths."""
import pickle

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib, anonymizer, f0_transforms, ops

CLEAN, M2O = "local/tuning/hifigan_clean.py", "local/tuning/hifigan_m2o.py"
STATE_BUFFER_BYTES = 900000


class SpeakerCMVN(nn.Module):
    """the inference side of satools.cmvn.SpeakerCMVN: the state buffer, its (de)serialisation, and the statistics as a device table"""

    def __init__(self):
        super().__init__()
        self.speaker_stats, self.stats_computed = {}, {}
        self.computed, self.keep_zeros = False, True
        self.register_buffer("model_state_buffer", torch.zeros(STATE_BUFFER_BYTES, dtype=torch.uint8))
        self._tables = {}

    def serialize_state(self):
        blob = pickle.dumps({"speaker_stats": self.speaker_stats, "stats_computed": self.stats_computed, "computed": self.computed,
                             "keep_zeros": self.keep_zeros})
        if len(blob) >= self.model_state_buffer.numel():
            raise RuntimeError(f"Not enough place {self.model_state_buffer.numel()} < {len(blob)} to store bytearray of SpeakerCMVN")
        self.model_state_buffer.zero_()
        self.model_state_buffer[:len(blob)] = torch.frombuffer(bytearray(blob), dtype=torch.uint8).to(self.model_state_buffer.device)

    def deserialize_state(self):
        """(a pickle inside the checkpoint, which load_model unpickles as a whole anyway: the same trust)"""
        state = pickle.loads(self.model_state_buffer.cpu().numpy().tobytes())
        self.speaker_stats, self.stats_computed = state["speaker_stats"], state["stats_computed"]
        self.computed, self.keep_zeros = state["computed"], state["keep_zeros"]
        self._tables = {}

    def _sync(self):
        """once per loaded buffer, at its first use (the reference: at its first forward); later calls read no device memory — a buffer
        is another one after load_state_dict (its version) or a move (its address)"""
        buf = self.model_state_buffer
        if self.__dict__.get("_seen") == (buf.data_ptr(), buf._version):
            return
        if int(buf[0]) != 0:
            self.deserialize_state()
            buf[0] = 0
        self.__dict__["_seen"] = (buf.data_ptr(), buf._version)

    def state_dict(self, *args, **kwargs):
        if self.speaker_stats:                            # (a buffer loaded and not yet read stays as it was loaded)
            self.serialize_state()
        return super().state_dict(*args, **kwargs)

    def require(self, speaker_id):
        self._sync()
        if not self.stats_computed.get(speaker_id, False):
            raise RuntimeError(f"Global statistics for speaker {speaker_id} must be computed before normalization.")

    def table(self, n_spk, device):
        """[n_spk, 2] = {mean, std} on `device`, built once per device; the float32 values the reference stored (torch.tensor(mean),
        sqrt(tensor(var + 1e-6))).  NaN rows for speakers without computed statistics (`require` refuses them first)"""
        self._sync()
        key = (str(device), int(n_spk))
        t = self._tables.get(key)
        if t is None:
            host = torch.full((n_spk, 2), float("nan"), dtype=torch.float32)
            for k, done in self.stats_computed.items():
                if done and str(k).isdigit() and int(k) < n_spk:
                    st = self.speaker_stats[k]
                    host[int(k), 0] = torch.as_tensor(st["mean"], dtype=torch.float32)
                    host[int(k), 1] = torch.as_tensor(st["std"], dtype=torch.float32)
            t = self._tables[key] = host.to(device)
        return t


def one_hot_index_str(row):
    """satools.utils.torch.get_one_hot_str_from_tensor"""
    index = torch.where(row == 1)
    return str(index[0][0].item()) if index[0].numel() > 0 else "Value not found"


def _variant(args, config):
    Base = anonymizer.build(args)

    class Net(Base):
        _config = config

        @property
        def convert_padded(self):               # hides the inherited method; the lookup goes on to __getattr__ below
            raise AttributeError("convert_padded")

        def __getattr__(self, name):
            if name == "convert_padded":        # (hasattr() is False: the batch job takes its plain convert branch)
                raise AttributeError(f"convert_padded is not built for the '{config}' config: hand the tracks over with set_f0 and call convert")
            return super().__getattr__(name)

        # ---- hooks of the shared class ---------------------------------------------------------------------------------------------
        def _statistics(self, f3, spk_id, dev):
            """-> (stats [n, 2] on the device, slice_stat: host list of one row per slice, or None)"""
            raise NotImplementedError

        def _spk_rows(self, spk_id, B, dev):
            if spk_id is None:
                return None
            if spk_id.is_cuda:
                spk = spk_id.to(device=dev, dtype=torch.float32).contiguous()
            else:
                spk = spk_id.to(torch.float32).contiguous().pin_memory().to(dev, non_blocking=True)
            assert B == spk.shape[0], \
                "len(target) != len(input_wav), check if the waveform batch size == target=len(['6081','4214'])"
            return spk

        def _forward(self, f0, bn, spk_id=None):
            dev = self._device()
            if dev.type != "cuda":
                raise _lib.SatError("the model is on the CPU: call .to('cuda') first (no CPU fallback)")
            f0_in = f0
            f0_d = f0_in.to(device=dev, dtype=torch.float32)
            if not f0_d.is_contiguous():
                f0_d = f0_d.contiguous()
            f3 = f0_d.unsqueeze(0) if f0_d.dim() == 2 else f0_d
            bn = bn.to(device=dev, dtype=torch.float32)              # whatever strides the extractor left: no copy
            B = bn.shape[0]
            if f3.dim() != 3 or f3.shape[0] != 1 or f3.shape[1] != B:
                # [S, R, T'] becomes R rows of S channels beside bn's B rows: torch.cat / conv_pre take S = 1 and R = B only
                raise RuntimeError(f"f0 of shape {tuple(f0_in.shape)} does not give one F0 row for each of the {B} rows of bn")
            spk = self._spk_rows(spk_id, B, dev)
            stats, slice_stat = self._statistics(f3, spk_id, dev)
            spec = args.f0_transformation
            if spec and "mean-reverv" in spec:
                # a moving average does not commute with the gather: the existing separate calls
                row = stats[slice_stat[0] if slice_stat else 0].contiguous()
                _lib.check(_lib.lib().sat_f0_apply_f32(_lib.ptr(f3), f3.numel(), _lib.ptr(row), 0, None, _lib.stream()), "sat_f0_apply_f32")
                if not (f0_in.is_cuda and f0_d.data_ptr() == f0_in.data_ptr()):
                    f0_in.copy_(f0_d)
                f0_t = self.f0_transformation(f3.permute(1, 0, 2).contiguous())
                n_spk = 0 if spk is None else spk.shape[1]
                x = ops.assemble_input(bn, f0_t.reshape(B, -1), spk, n_spk)
                ctx = ("calls", bn, f0_t, spk)
            else:
                quant = f0_transforms.parse_quant_bins(spec) if spec and "quant" in spec else 0
                noise = None
                if spec and "awgn" in spec:
                    noise = f0_transforms.draw_awgn((B, 1, f3.shape[-1]), f0_transforms.parse_awgn_db(spec)).to(torch.float32)
                    noise = noise.pin_memory().to(dev, non_blocking=True)
                x, norm = ops.generator_input(bn, f3, stats, slice_stat, quant, noise, spk)
                f0_in.copy_(norm.reshape(f0_in.shape))       # the reference leaves the normalised values in the caller's tensor
                ctx = ("fused", bn, norm, quant, noise, spk)
            y, _ = self.hifigan(x)
            if self._keep_ctx:            # convert(): the rows of near-tie utterances are assembled and generated again (_finish)
                self._fwd_ctx = ctx + (self.hifigan.last_arithmetic,)
            return y.to(torch.float32)

        def _reassemble(self, ctx, rows):
            if ctx[0] == "calls":
                _, bn, f0_t, spk, _ = ctx
                return ops.assemble_input(bn[rows], f0_t[rows].reshape(len(rows), -1).contiguous(), None if spk is None else spk[rows].contiguous(),
                                          0 if spk is None else spk.shape[1])
            # the same launch on the values the first one normalised: (v - 0) / 1 is v, then the same quantiser and the same noise
            _, bn, norm, quant, noise, spk, _ = ctx
            ident = torch.tensor([[0.0, 1.0]], dtype=torch.float32, device=bn.device)
            xs, _ = ops.generator_input(bn[rows], norm[:, rows].contiguous(), ident, None, quant, None if noise is None else noise[rows].contiguous(),
                                        None if spk is None else spk[rows].contiguous(), want_norm=False)
            return xs

    return Net


def build_clean(args):
    """build(args) -> Net(utt2spk) of local/tuning/hifigan_clean.py"""
    Base = _variant(args, CLEAN)

    class Net(Base):
        def __init__(self, utt2spk):
            super().__init__(utt2spk)
            self.f0_norm = SpeakerCMVN()
            self._modules["hifigan"] = self._modules.pop("hifigan")     # key order of the reference: bn_extractor, f0_norm, hifigan

        def _statistics(self, f3, spk_id, dev):
            ids = [one_hot_index_str(spk_id[i]) for i in range(f3.shape[0])]      # slice i <- spk_id[i]: in convert() the FIRST target alone
            for s in ids:
                self.f0_norm.require(s)
            return self.f0_norm.table(len(self.spk), dev), [int(s) for s in ids]

        def _calibration_input(self, bn, f0, B, dev):
            self.f0_norm._sync()
            k = next((int(s) for s, done in sorted(self.f0_norm.stats_computed.items(), key=lambda kv: int(kv[0])) if done), None)
            if k is None:
                raise RuntimeError("check_precision: no speaker of this checkpoint has computed F0 statistics")
            spk = F.one_hot(torch.full((B,), k, dtype=torch.long), num_classes=len(self.spk)).to(dev, torch.float32)
            x, _ = ops.generator_input(bn, f0, self.f0_norm.table(len(self.spk), dev), [k], 0, None, spk, want_norm=False)
            return x

    return Net


def build_m2o(args):
    """build(args) -> Net(utt2spk) of local/tuning/hifigan_m2o.py"""
    Base = _variant(args, M2O)

    class Net(Base):
        def __init__(self, utt2spk):
            super().__init__({})                    # no speakers: the generator reads 256 + 1 channels
            del self.spk, self.utt2spk

        def get_spk_id(self, wavinfo, target=None):
            return None

        def extract_features(self, x):
            keep, self.f0 = self.f0, None           # hifigan_m2o.py:63-66 never reads the track set_f0 left
            try:
                f0, bn, _ = super().extract_features(x, None)
            finally:
                self.f0 = keep
            return (f0, bn)

        def convert(self, x, defer_status=False):
            """hifigan_m2o.py:69-71; defer_status as in anonymizer.Net.convert"""
            self._defer_f0_status, self._f0_status, self._bn_fix = True, None, None
            try:
                (f0, bn) = self.extract_features(x)
            finally:
                self._defer_f0_status = False
            fix, self._bn_fix = self._bn_fix, None
            self._keep_ctx = fix is not None
            try:
                y = self._forward(f0, bn)
            finally:
                self._keep_ctx = False
            st, self._f0_status = self._f0_status, None
            return self._finish(y, st, fix, defer_status)

        def _statistics(self, f3, spk_id, dev):
            stats = torch.empty(1, 2, dtype=torch.float32, device=dev)      # UttCMVN(var_norm=True, keep_zeros=True): batch-coupled
            _lib.check(_lib.lib().sat_f0_stats_f32(_lib.ptr(f3), f3.numel(), _lib.ptr(stats), _lib.stream()), "sat_f0_stats_f32")
            return stats, None

        def _calibration_input(self, bn, f0, B, dev):
            stats, _ = self._statistics(f0, None, dev)
            x, _ = ops.generator_input(bn, f0, stats, None, 0, None, None, want_norm=False)
            return x

        def forward(self, egs_with_feat):
            return self._forward(egs_with_feat["get_f0"], egs_with_feat["get_bn"])

    return Net
