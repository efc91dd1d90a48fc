"""Helpers of the variant-board tests (Connect4 6x5 "connect4_6_5" and 8x7 "connect4_8_7").

The oracle (oracle/) and tests/parity_helpers.py know the two default games only.  `variant_oracle` teaches
them the variant names for the duration of a test: make_env of oracle.mcts / oracle.selfplay /
oracle.hardcoded returns oracle.envs.Connect4Env(w, h) for them and parity_helpers' A_OF / CELLS_OF gain the two
names; both are undone afterwards.  With it g2_tape, g2_threaded, g3_tapes, g5_tapes and run_g*_group work on
the variant fixtures as they are.  A test module imports the fixture by name.
"""
import pytest

# tag of the fixture files -> (game name, width, height)
BOARDS = {"c4_6x5": ("connect4_6_5", 6, 5), "c4_8x7": ("connect4_8_7", 8, 7)}
SIZE_OF = {game: (w, h) for game, w, h in BOARDS.values()}
TAGS = sorted(BOARDS)


@pytest.fixture
def variant_oracle():
    import oracle.envs
    import oracle.hardcoded
    import oracle.mcts
    import oracle.selfplay
    from tests import parity_helpers as ph

    mods = (oracle.mcts, oracle.selfplay, oracle.hardcoded)
    saved = [m.make_env for m in mods]
    base = oracle.envs.make_env

    def make_env(game):
        if game in SIZE_OF:
            return oracle.envs.Connect4Env(*SIZE_OF[game])
        return base(game)

    for m in mods:
        m.make_env = make_env
    for game, (w, h) in SIZE_OF.items():
        ph.A_OF[game] = w
        ph.CELLS_OF[game] = w * h
    try:
        yield make_env
    finally:
        for m, f in zip(mods, saved):
            m.make_env = f
        for game in SIZE_OF:
            ph.A_OF.pop(game, None)
            ph.CELLS_OF.pop(game, None)


def searches(tag):
    from tests.parity_helpers import load_json

    return load_json(f"mcts_search_{tag}.json")


def selfplay_games(tag):
    from tests.parity_helpers import load_json

    return load_json(f"selfplay_games_{tag}.json")


def arena_games(tag):
    from tests.parity_helpers import load_json

    return load_json(f"arena_games_{tag}.json")
