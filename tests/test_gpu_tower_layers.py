"""The C = 128 7x6 trunk reproduces, bit for bit, the outputs recorded from the library of the commit before its
second-buffer layers were reworked (buffer-relative operand offsets, the fp16 residual add as one mixed-precision
FMA per element): tests/golden/tower_c128_parent_bits.npz, written by tests/golden/gen_tower_c128_parent_bits.py
with that commit's library.  13 boards (two full 6-board tiles and one with a single board), nets of 1, 2 and 20
blocks, fp16 and bf16, the host-count path and the device-count path at counts 1, 6, 7 and 13."""
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("gen_tower_c128_parent_bits",
                                               os.path.join(_GOLDEN, "gen_tower_c128_parent_bits.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)


@pytest.fixture(scope="module")
def recorded():
    with np.load(os.path.join(_GOLDEN, "tower_c128_parent_bits.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def current():
    return gen.outputs()


def test_fixture_holds_every_case(recorded):
    paths = ["host"] + [f"{kind}{n}" for n in gen.COUNTS for kind in ("dev", "pack")]
    want = {f"{d}_b{b}_{path}_{o}" for d in gen.DTYPES for b in gen.BLOCKS for path in paths for o in "pv"}
    assert set(recorded) == want
    assert recorded["fp16_b20_host_p"].shape == (gen.BOARDS, 7) and recorded["fp16_b20_host_v"].shape == (gen.BOARDS,)


@pytest.mark.parametrize("blocks", gen.BLOCKS)
@pytest.mark.parametrize("dtype", gen.DTYPES)
def test_trunk_bits_match_parent(recorded, current, dtype, blocks):
    keys = [k for k in recorded if k.startswith(f"{dtype}_b{blocks}_")]
    assert len(keys) == 2 * (1 + 2 * len(gen.COUNTS))
    for k in keys:
        assert np.isfinite(recorded[k]).all(), k
        assert torch.equal(torch.from_numpy(current[k]), torch.from_numpy(recorded[k])), k
