"""Shared by the sample_pairs tests: tools/emulate_select_sample.py as a module, and the expected sample of a frame."""
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_emu = None


def emulator():
    """tools/emulate_select_sample.py as a module (the key, the strata, the definition and the emulated passes)."""
    global _emu
    if _emu is None:
        spec = importlib.util.spec_from_file_location("emulate_select_sample",
                                                      os.path.join(ROOT, "tools", "emulate_select_sample.py"))
        _emu = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(_emu)
    return _emu


def expected_sample(pdf, edges, quota, seed, eligible=None):
    """The sample of the parent frame `pdf` (its row position is the pair's ordinal) by the definition: (the expected
    frame with stratum and sampling_weight, the expected strata() columns pairs and sampled)."""
    emu = emulator()
    mp = pdf["match_probability"].to_numpy(dtype=np.float64)
    kept, stratum, pop, cnt = emu.sample(seed, np.arange(len(pdf), dtype=np.int64), mp, edges, quota, eligible)
    exp = pdf[kept].reset_index(drop=True)
    b = stratum[kept]
    exp["stratum"] = b.astype(np.int32)
    exp["sampling_weight"] = pop[b].astype(np.float64) / cnt[b].astype(np.float64)
    return exp, pop, cnt
