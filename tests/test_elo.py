"""CPU: the rating layer (self_play_reinforcement_learning_amd/elo.py): the deterministic Elo fit in closed form
and against the reference's own SGD fit (tests/golden/elo_fit.json, written by tests/golden/make_elo_golden.py),
the ModelDatabase's files, and the league's pairing-to-slot schedule."""
import json
import math
import os

import pytest
import torch

from self_play_reinforcement_learning_amd import Elo, ModelDatabase
from self_play_reinforcement_learning_amd.base_model import ModelContainer
from self_play_reinforcement_learning_amd.elo import fit_elo, result_key
from self_play_reinforcement_learning_amd.envs import Connect4Env
from self_play_reinforcement_learning_amd.hardcoded_players import OneStepLookahead, Random
from self_play_reinforcement_learning_amd.modules import ResidualTower


@pytest.mark.parametrize("w,d,l", [(60, 10, 30), (100, 0, 0), (0, 0, 100), (1, 98, 1), (33, 34, 33)])
def test_two_models_closed_form(w, d, l):
    """With the default prior (one virtual draw) the maximum has the closed form E = score / games."""
    r = fit_elo(["random", "m"], {"random__m": dict(wins=w, draws=d, losses=l)}, "random")
    want = 400 * math.log10((w + d / 2 + 0.5) / (l + d / 2 + 0.5))
    assert r["random"] == 0
    assert abs((r["random"] - r["m"]) - want) < 1e-6, (r, want)
    # the anchor's rating only shifts the answer
    r2 = fit_elo(["random", "m"], {"random__m": dict(wins=w, draws=d, losses=l)}, "m", anchor_elo=1000)
    assert r2["m"] == 1000 and abs((r2["random"] - r2["m"]) - want) < 1e-6


def test_one_sided_table_without_prior_has_no_fit():
    with pytest.raises(RuntimeError):
        fit_elo(["random", "m"], {"random__m": dict(wins=0, draws=0, losses=100)}, "random", prior_draws=0)


def test_four_models_against_the_reference_fit(golden_dir):
    """The deterministic fit of the reference's likelihood (prior_draws=0) lies within 3 x the recorded
    seed-to-seed deviation of the mean of the reference's five SGD runs, per model (3 x: the reference's SGD
    still moves by a fraction of a point per step at its final learning rate)."""
    g = json.load(open(os.path.join(golden_dir, "elo_fit.json")))
    fit = fit_elo(g["models"], g["table"], g["anchor"], anchor_elo=0, prior_draws=0)
    bound = 3 * g["max_deviation"]
    for m, mean in zip(g["models"], g["mean"]):
        print(m, "fit", fit[m], "reference mean", mean, "bound", bound)
    for m, mean in zip(g["models"], g["mean"]):
        assert abs(fit[m] - mean) <= bound, (m, fit[m], mean, bound)
    # the same maximum from the gradient's side: every model's expected score equals its actual score
    for m in g["models"]:
        actual = expected = 0.0
        for key, r in g["table"].items():
            a, b = key.split("__")
            if m not in (a, b):
                continue
            n = r["wins"] + r["draws"] + r["losses"]
            s = r["wins"] + r["draws"] / 2
            e = n / (1 + 10 ** ((fit[b] - fit[a]) / 400))
            actual += s if m == a else n - s
            expected += e if m == a else n - e
        if m != g["anchor"]:
            assert abs(actual - expected) < 1e-6, (m, actual, expected)


def _net():
    torch.manual_seed(1)
    return ResidualTower(7, 6, 7, num_blocks=1, filter_factor=8)


def test_database_round_trip(tmp_path):
    db = ModelDatabase(tmp_path / "db", Connect4Env)
    net = _net()
    db.add_model("net1", ModelContainer(policy_gen="MCTreeSearch",
                                        policy_kwargs=dict(network=net, iterations=40, alpha=0.5, strong_play=True,
                                                           memory_queue=object())))
    db.add_model("random", ModelContainer(Random))
    db.add_model("look", ModelContainer(OneStepLookahead))
    # a second handle on the same directory reads everything back from the files
    db2 = ModelDatabase(tmp_path / "db", Connect4Env)
    assert list(db2.models()) == ["net1", "random", "look"]
    e = db2.models()["net1"]
    assert e["policy"] == "MCTreeSearch"
    assert e["policy_kwargs"] == dict(iterations=40, alpha=0.5, strong_play=True)
    assert e["net"] == dict(width=7, height=6, action_size=7, num_blocks=1, filter_factor=8)
    back = db2.network("net1")
    for k, v in net.state_dict().items():
        assert torch.equal(back.state_dict()[k], v), k
    c = db2.get_model("random")
    assert c.policy_gen is Random
    assert db2.network("random") is None
    players = Elo(db2).players(["net1", "random", "look"])
    assert players[0]["iterations"] == 40 and players[0]["alpha"] == 0.5 and players[0]["strong_play"] is True
    assert players[1] == dict(kind="random") and players[2] == dict(kind="lookahead")
    assert db2.elos() == {}
    with pytest.raises(KeyError):
        db2.get_model("nobody")


def test_database_refuses_taken_and_underscored_names(tmp_path):
    db = ModelDatabase(tmp_path, Connect4Env)
    db.add_model("random", ModelContainer(Random))
    with pytest.raises(ValueError):
        db.add_model("random", ModelContainer(Random))
    with pytest.raises(ValueError):
        db.add_model("my_model", ModelContainer(Random))
    assert list(db.models()) == ["random"]


def test_results_accumulate_under_the_reference_key_order(tmp_path):
    db = ModelDatabase(tmp_path, Connect4Env)
    for n in ("random", "a", "b"):
        db.add_model(n, ModelContainer(Random))
    elo = Elo(db)
    assert result_key("a", "random") == ("random__a", True) and result_key("b", "a") == ("b__a", False)
    b1 = {"first": dict(wins=3, draws=1, losses=0), "second": dict(wins=2, draws=0, losses=2)}
    elo.accumulate([("a", "random"), ("b", "a")], [b1, b1])
    assert db.results() == {"random__a": dict(wins=2, draws=1, losses=5), "b__a": dict(wins=5, draws=1, losses=2)}
    elo.accumulate([("a", "random")], [b1])
    assert db.results()["random__a"] == dict(wins=4, draws=2, losses=10)
    r = elo.calculate_elo()
    assert r["random"] == 0 and all(math.isfinite(x) for x in r.values())
    assert r["b"] > r["a"] > r["random"]
    assert db.elos() == {"elo": r}


def test_disconnected_results_raise(tmp_path):
    db = ModelDatabase(tmp_path, Connect4Env)
    for n in ("random", "a", "b", "c"):
        db.add_model(n, ModelContainer(Random))
    elo = Elo(db)
    b = {"first": dict(wins=3, draws=1, losses=1), "second": dict(wins=2, draws=1, losses=2)}
    elo.accumulate([("a", "random"), ("b", "c")], [b, b])  # b and c never meet random or a
    with pytest.raises(ValueError, match="b, c"):
        elo.calculate_elo()
    elo.accumulate([("c", "a")], [b])
    assert set(elo.calculate_elo()) == {"random", "a", "b", "c"}


def test_command_line_calculate_elo(tmp_path, capsys):
    """`python -m self_play_reinforcement_learning_amd.elo calculate_elo --dir D --g connect4 --b 6 5`."""
    from self_play_reinforcement_learning_amd import elo as elo_mod

    db = ModelDatabase(tmp_path, Connect4Env(6, 5))
    for n in ("random", "a"):
        db.add_model(n, ModelContainer(Random))
    Elo(db).accumulate([("a", "random")], [{"first": dict(wins=4, draws=0, losses=0),
                                            "second": dict(wins=3, draws=1, losses=0)}])
    elo_mod.main(["calculate_elo", "--dir", str(tmp_path), "--g", "connect4", "--b", "6", "5"])
    printed = json.loads(capsys.readouterr().out)
    assert printed == db.elos()["elo"]
    assert printed["random"] == 0 and abs(printed["a"] - 400 * math.log10(8.0 / 1.0)) < 1e-6


@pytest.mark.parametrize("games,g", [(8, 8), (7, 8), (1, 2), (100, 100)])
def test_league_schedule(games, g):
    """Pairing p owns slots [p g, (p + 1) g), g even: swap_sides = slot odd, so each side is first in g / 2."""
    from self_play_reinforcement_learning_amd.engine import league_schedule

    pairings = [(0, 1), (0, 2), (1, 2)]
    got_g, sched = league_schedule(pairings, games)
    assert got_g == g and g % 2 == 0
    assert sched == [(p * g, i, j) for p, (i, j) in enumerate(pairings)]
    for first, _, _ in sched:
        slots = range(first, first + g)
        assert sum(s % 2 for s in slots) == g // 2  # swapped games: the second player moves first
