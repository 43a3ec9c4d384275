#!/usr/bin/env python3
"""The reference's own word on the YAAPT edge cases of tests/yaapt_cases.py, made by IMPORTING THE REFERENCE in the build
container like make_fixtures.py (whose helpers this script uses).  Run from the repo root:
    python tests/golden/make_f0_edge_fixtures.py

Every catalogue case inside the entry point's 4..2048 frames goes through the reference's `yaapt(wav, opts)`
(satools/hifigan/yaapt.py:946-951, one thread as that module sets on import).  Data only is written:
  fx_f0_edges.npz    <case name>         the F0 track [1, nframes], float32              (the reference returned)
                     raised/<case name>  the exception's type name as a string, else ""  (every case)
  fx_f0_options.npz  the same two entries for every (case, option set) pair of yaapt_cases.recorded_cases(), each run with the
                     options of its set, and
                     assert/<case name>  whether the raised error's text names the reference's `assert N > 0` of crs_corr
A torch.jit.script function reports a Python-level assert or a failed tensor operation as its own exception classes;
what is recorded is the name of the first class in the raised exception's MRO that the builtins know (RuntimeError for
torch.jit.Error), which is what a caller can catch without importing torch internals."""
import builtins
import os
import sys

import numpy as np

from make_fixtures import F0_OPTS, GOLD, ROOT, setup_reference


def builtin_name(exc):
    for cls in type(exc).__mro__:
        if getattr(builtins, cls.__name__, None) is cls:
            return cls.__name__
    return type(exc).__name__


def main():
    setup_reference()
    import torch
    from satools.hifigan import yaapt as ref_yaapt      # the reference (sets one thread)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import yaapt_cases
    assert yaapt_cases.OPTS == F0_OPTS
    out = {}
    for case in yaapt_cases.CASES:
        if case.refused:
            continue
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
        print(f"{case.name:28s} raised={raised!r:16s} voiced frames={int((out[case.name] > 0).sum()) if not raised else '-'}"
              + ("" if raised == want else f"   !! the catalogue says {want!r}"))
    np.savez_compressed(os.path.join(GOLD, "fx_f0_edges.npz"), **out)
    print("wrote fx_f0_edges.npz:", os.path.getsize(os.path.join(GOLD, "fx_f0_edges.npz")), "bytes")

    # the option sets: every (case, set) pair of the catalogue, the ones the reference raises on included
    out = {}
    for case in yaapt_cases.recorded_cases():
        wav = case.wav().unsqueeze(0)
        try:
            track = ref_yaapt.yaapt(wav, dict(case.opts))
            raised, message = "", ""
            out[case.name] = track.numpy().astype(np.float32)
            assert case.nframes is None or out[case.name].shape == (1, case.nframes), (case, out[case.name].shape)
        except Exception as e:                           # noqa: BLE001  (the type is the recorded result)
            raised, message = builtin_name(e), str(e)
        out["raised/" + case.name] = np.array(raised)
        # a scripted function reports a Python assert as torch.jit.Error (a RuntimeError) whose text names the original class
        out["assert/" + case.name] = np.array("AssertionError: ERROR: Negative index in the cross correlation" in message)
        print(f"{case.name:48s} raised={raised!r:16s} voiced frames={int((out[case.name] > 0).sum()) if not raised else '-'}"
              + (f"   {message.strip().splitlines()[-1][:100]}" if raised else ""))
    np.savez_compressed(os.path.join(GOLD, "fx_f0_options.npz"), **out)
    print("wrote fx_f0_options.npz:", os.path.getsize(os.path.join(GOLD, "fx_f0_options.npz")), "bytes")


if __name__ == "__main__":
    main()
