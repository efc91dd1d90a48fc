"""Generator of tower_c128_parent_bits.npz: the C = 128 7x6 fused trunk's outputs on 13 boards, recorded from the
library of the commit before the trunk's second-buffer layers were made as cheap as its first-buffer ones.  That
change is arithmetic-neutral (operand addressing, and a residual add of the same single rounding), so
tests/test_gpu_tower_layers.py holds every later library to these bits.

  SPMCTS_LIB=<that commit's libspmcts.so> python tests/golden/gen_tower_c128_parent_bits.py [OUT.npz]

Needs a GPU.  outputs() is also what the test computes with the current library."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
BOARDS = 13  # two full 6-board tiles and a tile with one board: the empty-slot rows are covered
BLOCKS = (1, 2, 20)  # one layer of each parity / the smallest repeat of the loop body / the workload's depth
DTYPES = ("fp16", "bf16")
COUNTS = (1, 6, 7, 13)  # device-count launches: part of a tile, a full tile, a tile + 1, all


def outputs():
    """{key: float32 array}: probabilities p and values v of the host-count path (`host`) and of the device-count
    path for each count of COUNTS, round-aligned (`dev`) and packed (`pack`) launches, per (dtype, blocks)."""
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import torch

    from self_play_reinforcement_learning_amd.evaluator import HipTowerEvaluator
    from tests.test_gpu_tower import _net, _planes

    x = _planes(7, 6, BOARDS, seed=5).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    res = {}
    for blocks in BLOCKS:
        net = _net(7, 6, 7, blocks, 32, seed=0)
        for name in DTYPES:
            hip = HipTowerEvaluator(net, dtype={"fp16": torch.float16, "bf16": torch.bfloat16}[name])
            p, v = hip(x)
            res[f"{name}_b{blocks}_host_p"], res[f"{name}_b{blocks}_host_v"] = p, v.view(-1)
            for n in COUNTS:
                cnt = torch.tensor([n], dtype=torch.int32, device=x.device)
                for pack in (False, True):
                    hip.concurrent = pack
                    pd, vd = hip.forward_dev(x, cnt, BOARDS)
                    torch.cuda.synchronize()
                    key = f"{name}_b{blocks}_{'pack' if pack else 'dev'}{n}"
                    res[key + "_p"], res[key + "_v"] = pd[:n].clone(), vd[:n].view(-1).clone()
    return {k: t.float().cpu().numpy() for k, t in res.items()}


if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                                             "tower_c128_parent_bits.npz")
    res = outputs()
    np.savez_compressed(out, **res)
    print(f"{out}: {len(res)} arrays, {os.path.getsize(out)} bytes")
