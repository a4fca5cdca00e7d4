"""Host side of the CU-count knob (no GPU): engine.best_chunk's choice over explicit CU counts by brute force over its own cost model, and the
parsing of VISREP_RESERVE_CUS / visrep_set_reserved_cus (pure host state of the library: no device call is involved)."""
import os
import subprocess
import sys

import pytest

from law_of_vision_representation_in_mllms_amd import _lib, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _efficiency(count, tokens, d, cus):
    """engine.best_chunk's cost model restated: tiles over paid tile slots of a [count * tokens, d] GEMM on `cus` CUs, the tail launch priced as
    its docstring says (0.45 of a round plus twice its share of one).  This pins the CHOICE (range, near-best, largest), not that the model still
    follows visrep_gemm_dispatch: the head / tail rule itself is pinned on the GPU by GEMM_PLAN in tests/test_gpu_cu_counts.py."""
    ntn = max(1, d // 256)
    tiles = (count * tokens + 255) // 256 * ntn
    rounds, rem = tiles // cus, tiles % cus
    if rem == 0:
        paid = float(rounds)
    elif rounds >= 1 and 4 * rem <= cus and (rounds * cus) % ntn == 0:
        paid = rounds + 0.45 + 2.0 * rem / cus
    else:
        paid = rounds + 1.0
    return tiles / (cus * paid)


@pytest.mark.parametrize("tokens,d", [(577, 1024), (257, 1024), (729, 1152), (257, 768)])
@pytest.mark.parametrize("cap", [128, 64, 37])
def test_best_chunk_over_explicit_cu_counts(tokens, d, cap):
    """For every CU count a reservation can leave (64 .. 256 in steps of 8) and the four production (tokens, width) pairs: the chunk lies in
    [cap // 2, cap], its efficiency is within 0.01 (absolute: the function's reading of "within 1 %", efficiencies being at most 1) of the brute-force best of that
    range, and no larger count is."""
    for cus in range(64, 257, 8):
        got = engine.best_chunk(tokens, d, cap, cus=cus)
        lo = max(cap // 2, 1)
        assert lo <= got <= cap, (cus, got)
        effs = {c: _efficiency(c, tokens, d, cus) for c in range(lo, cap + 1)}
        top = max(effs.values())
        assert effs[got] >= top - 0.01, (cus, got, effs[got], top)
        assert all(effs[c] < top - 0.01 for c in range(got + 1, cap + 1)), (cus, got)
    assert engine.best_chunk(577, 1024, 128, cus=256) == 113 and engine.best_chunk(257, 1024, 128, cus=256) == 127      # the documented values


def test_set_reserved_cus_clamps_rounds_and_returns_the_previous_value():
    lib = _lib.load()
    start = lib.visrep_set_reserved_cus(0)
    try:
        assert lib.visrep_set_reserved_cus(-7) == 0                   # negative -> 0
        assert lib.visrep_set_reserved_cus(13) == 0                   # 13 -> 8
        assert lib.visrep_set_reserved_cus(16) == 8
        assert lib.visrep_set_reserved_cus(23) == 16                  # 23 -> 16
        assert lib.visrep_set_reserved_cus(200) == 16                 # stored as given (a multiple of 8); the floor is applied where the count is read
        assert lib.visrep_set_reserved_cus(0) == 200
    finally:
        lib.visrep_set_reserved_cus(start)


_CHILD = """
import os, sys
sys.path.insert(0, {root!r})
from law_of_vision_representation_in_mllms_amd import _lib
lib = _lib.load()
first = lib.visrep_set_reserved_cus(40)          # returns what the environment said, parsed on this first use
os.environ["VISREP_RESERVE_CUS"] = "64"          # a later change of the environment is not read again
second = lib.visrep_set_reserved_cus(0)
third = lib.visrep_set_reserved_cus(0)
print(first, second, third)
"""


@pytest.mark.parametrize("env,first", [("16", 16), ("13", 8), ("-24", 0), ("", 0), (None, 0), ("junk", 0)])
def test_reserve_cus_environment_is_parsed_once(env, first):
    """VISREP_RESERVE_CUS in a fresh process: clamped to >= 0 and rounded down to a multiple of 8 like the setter's argument, read on first use
    only."""
    e = {k: v for k, v in os.environ.items() if k != "VISREP_RESERVE_CUS"}
    if env is not None:
        e["VISREP_RESERVE_CUS"] = env
    out = subprocess.run([sys.executable, "-c", _CHILD.format(root=ROOT)], env=e, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split() == [str(first), "40", "0"], out.stdout
