"""Generate tests/golden/elo_fit.json by running the REFERENCE's own rating fit.

Run in the build container only (needs /root/reference), with make_golden.py's conventions: the reference is
imported by path through tests/golden/refshims, nothing of it is copied, and only the input table and the
outputs it produced are written.

    python tests/golden/make_elo_golden.py

The reference's Elo.calculate_elo (games/algos/elo.py:93-137) is 100,000 SGD steps on batches of 32 sampled
from the result table, from a random initial rating vector, so its answer depends on the torch and numpy
seeds.  It is run on one fixed, non-separable 4-model table (every pair has wins, draws and losses, so the
likelihood has a finite maximum) under five seeds; dict objects stand in for its three shelves.  Written: the
table, the five rating vectors, their mean per model and the largest deviation of any run from that mean.
tests/test_elo.py holds the deterministic fit (prior_draws=0: the same likelihood) against the mean.
"""
import json
import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, os.path.join(HERE, "refshims"))
sys.path.insert(0, REF)

import torch  # noqa: E402

MODELS = ["random", "a", "b", "c"]  # registration order (the reference's model_shelf keys)
# "x__y" with x > y, in x's view (elo.py:49-71)
TABLE = {
    "random__a": {"wins": 12, "draws": 6, "losses": 82},
    "random__b": {"wins": 5, "draws": 4, "losses": 91},
    "random__c": {"wins": 3, "draws": 2, "losses": 95},
    "b__a": {"wins": 58, "draws": 14, "losses": 28},
    "c__a": {"wins": 71, "draws": 9, "losses": 20},
    "c__b": {"wins": 49, "draws": 21, "losses": 30},
}
SEEDS = [0, 1, 2, 3, 4]


class _Database:
    """What Elo.calculate_elo reads of a ModelDatabase: three mappings and a Memory."""

    def __init__(self, memory):
        self.model_shelf = {m: None for m in MODELS}
        self.result_shelf = {k: dict(v) for k, v in TABLE.items()}
        self.elo_value_shelf = {}
        self.memory = memory


def main():
    os.chdir("/tmp")  # reference modules may write logs into cwd
    if "torch.utils.tensorboard" not in sys.modules:
        try:
            import importlib

            importlib.import_module("torch.utils.tensorboard")  # elo.py imports the scheduler, which imports it
        except ImportError:  # not installed: the fit never touches it
            import types

            stub = types.ModuleType("torch.utils.tensorboard")
            stub.SummaryWriter = object
            sys.modules["torch.utils.tensorboard"] = stub
    import games.algos.elo as ref_elo
    from rl_utils.memory import Memory

    # The reference's calculate_elo ends with `elo_net.elo_vals.weight.tolist()[model_indices[model]]`
    # (elo.py:131-133): the weight is [1, n - 1], so with more than two models that raises IndexError after the
    # whole fit has run.  The fitted network is kept here so its ratings can be read all the same: the
    # reference's class is subclassed only to remember the instance, its arithmetic is untouched.
    made = []

    class Remembered(ref_elo.EloNetwork):
        def __init__(self, *args, **kwargs):
            super().__init__(*args, **kwargs)
            made.append(self)

    ref_elo.EloNetwork = Remembered
    free = [m for m in MODELS if m != "random"]  # the reference's model_indices order
    runs = []
    for seed in SEEDS:
        torch.manual_seed(seed)
        np.random.seed(seed)
        random.seed(seed)
        try:
            ratings = ref_elo.Elo(_Database(Memory())).calculate_elo(anchor_model="random", anchor_elo=0)
        except IndexError:
            w = made[-1].elo_vals.weight.detach().reshape(-1).tolist()
            ratings = dict(zip(free, w), random=0.0)
        runs.append([float(ratings[m]) for m in MODELS])
        print(seed, runs[-1], flush=True)
    arr = np.asarray(runs, dtype=np.float64)
    mean = arr.mean(0)
    out = {"models": MODELS, "anchor": "random", "table": TABLE, "seeds": SEEDS, "ratings": runs,
           "mean": mean.tolist(), "max_deviation": float(np.abs(arr - mean).max())}
    with open(os.path.join(HERE, "elo_fit.json"), "w") as f:
        json.dump(out, f, indent=1)
    print("mean", out["mean"], "max deviation", out["max_deviation"])


if __name__ == "__main__":
    main()
