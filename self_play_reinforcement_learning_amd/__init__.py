"""MI355X-native batched self-play MCTS (drop-in for reubenvanammers/self_play_reinforcement_learning's
games/algos/mcts.py + games/algos/self_play_parallel.py hot path).

Public API mirrors the reference:
    MCTreeSearch, Move                    (games/algos/mcts.py)
    SelfPlayScheduler                     (games/algos/self_play_parallel.py)
    Memory                                (rl_utils/memory.py)
    ModelContainer, BasePlayer, Policy    (games/general/base_model.py)
    ResidualTower                         (games/general/modules.py)
    Connect4Env, TicTacToeEnv             (games/connect4, games/tictactoe)
    OneStepLookahead, Random              (games/general/hardcoded_players.py)
    Negamax                               (no reference form: looks `depth` plies ahead, exactly)
    Elo, ModelDatabase                    (games/algos/elo.py, games/algos/model_database.py)
plus the arena itself: Arena, SelfPlayEngine, LanedEngine, LeagueEngine, DeviceTableNet, and what the reference
has no form of: opening books (openings.py: enumerate_openings, validate_openings), analyse_positions, and the
exact depth-limited solver (solve_positions, tactical_report), and the exact solver to the end of the game
(solve.py: SolveTable, solve_to_end, perfect_report) with the reference's PerfectEvaluator
(games/algos/evaluation_worker.py) on top of it, and game records (records.py: GameRecords, the move lists the
arenas' games leave behind with record_games=True; grade_games, their moves held against the exact solvers), and
the search trees below the root (tree.py: TreeView over Arena.export_subtrees; Arena.pv_batch,
MCTreeSearch.principal_variation / .tree), and what a search tree has proved about its position (Arena.bounds_batch,
MCTreeSearch.score_bounds, TreeView.score_bounds; tree.py: bounds_to_codes, classify_bounds, describe_bounds), and
playing it (proof_play= of MCTreeSearch / SelfPlayEngine / a LeagueEngine player: Arena.set_proof_play,
proof_moves_batch, proof_last, proof_stats, proof_stop; tree.proof_move_set, the keep set's host twin), and keeping
the bounds in the nodes (stored_bounds= of MCTreeSearch / SelfPlayEngine: Arena.set_stored_bounds,
Arena.export_subtrees(bounds=True), TreeView.node_bounds), and searching with them (solver_search= of MCTreeSearch /
SelfPlayEngine / LanedEngine / a LeagueEngine player / analyse_positions: Arena.set_solver_rules, solver_stats;
tree.solver_select, the two rules' host form), and the boards' mirror symmetry (symmetry.py: mirror_boards,
mirror_actions, mirror_probs, mirror_moves, canonical, library_canonical, SymmetricNet; symmetry="mirror" of
MCTreeSearch / the engines / analyse_positions: Arena.set_symmetry; DeviceReplay.sample_batch(mirror=True),
deduplicate(symmetric=True)).
"""
from .base_model import BasePlayer, ModelContainer, Policy, TrainableModel  # noqa: F401
from .memory import Memory  # noqa: F401
from .modules import InferenceTower, ResidualTower  # noqa: F401

_LAZY = {
    "Arena": ".arena",
    "SelfPlayEngine": ".engine",
    "LanedEngine": ".engine",
    "LeagueEngine": ".engine",
    "Elo": ".elo",
    "ModelDatabase": ".elo",
    "DeviceTableNet": ".evaluator",
    "make_evaluator": ".evaluator",
    "MCTreeSearch": ".mcts",
    "Move": ".mcts",
    "analyse_positions": ".mcts",
    "solve_positions": ".mcts",
    "tactical_report": ".mcts",
    "SolveTable": ".solve",
    "solve_to_end": ".solve",
    "perfect_report": ".solve",
    "PerfectEvaluator": ".evaluation_worker",
    "GameRecords": ".records",
    "grade_games": ".records",
    "TreeView": ".tree",
    "bounds_to_codes": ".tree",
    "classify_bounds": ".tree",
    "describe_bounds": ".tree",
    "proof_move_set": ".tree",
    "solver_select": ".tree",
    "enumerate_openings": ".openings",
    "validate_openings": ".openings",
    "mirror_boards": ".symmetry",
    "mirror_actions": ".symmetry",
    "mirror_probs": ".symmetry",
    "mirror_moves": ".symmetry",
    "canonical": ".symmetry",
    "library_canonical": ".symmetry",
    "SymmetricNet": ".symmetry",
    "SelfPlayScheduler": ".self_play_parallel",
    "Connect4Env": ".envs",
    "TicTacToeEnv": ".envs",
    "GameOver": ".envs",
    "OneStepLookahead": ".hardcoded_players",
    "Random": ".hardcoded_players",
    "Negamax": ".hardcoded_players",
}


def __getattr__(name):
    if name in _LAZY:
        import importlib

        mod = importlib.import_module(_LAZY[name], __name__)
        return getattr(mod, name)
    raise AttributeError(name)
