#!/usr/bin/env python3
"""The reference's own word on the wide option sets of tests/yaapt_wide_cases.py (frames of time_track that overlap more than their
predecessor: the reference's default options among them), made by IMPORTING THE REFERENCE in the build container like
make_f0_edge_fixtures.py (whose helpers this script uses).  Run from the repo root:
    python tests/golden/make_f0_wide_fixtures.py

Every case of the accepted sets goes through the reference's `yaapt(wav, opts)` (satools/hifigan/yaapt.py:946-951, one thread as that
module sets on import) with the options of its set.  Data only is written:
  fx_f0_wide.npz   <case name>         the F0 track [1, nframes], float32              (the reference returned)
                   raised/<case name>  the exception's type name as a string, else ""  (every case)"""
import os
import sys

import numpy as np

from make_f0_edge_fixtures import builtin_name
from make_fixtures import GOLD, ROOT, setup_reference


def main():
    setup_reference()
    from satools.hifigan import yaapt as ref_yaapt      # the reference (sets one thread)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import yaapt_wide_cases as ywc
    out = {}
    for case in ywc.recorded():
        wav = case.wav().unsqueeze(0)
        try:
            track = ref_yaapt.yaapt(wav, dict(case.opts))
            raised = ""
            out[case.name] = track.numpy().astype(np.float32)
            assert out[case.name].shape == (1, case.nframes), (case, out[case.name].shape)
        except Exception as e:                           # noqa: BLE001  (the type is the recorded result)
            raised = builtin_name(e)
        out["raised/" + case.name] = np.array(raised)
        want = case.raises or ""
        print(f"{case.name:32s} frames={case.nframes} raised={raised!r:16s} voiced frames={int((out[case.name] > 0).sum()) if not raised else '-'}"
              + ("" if raised == want else f"   !! the catalogue says {want!r}"), flush=True)
    np.savez_compressed(os.path.join(GOLD, "fx_f0_wide.npz"), **out)
    print("wrote fx_f0_wide.npz:", os.path.getsize(os.path.join(GOLD, "fx_f0_wide.npz")), "bytes")


if __name__ == "__main__":
    main()
