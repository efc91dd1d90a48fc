"""`PerfectEvaluator` (games/algos/evaluation_worker.py): "N correct moves out of M positions" against a perfect
player.  The reference asks an external Connect4 solver and its opening book; here the perfect player is the
exact solver to the end of the game (solve.py: solve_to_end on the device), so any instantiated board works and
nothing outside the package is needed.

The positions are searched in one arena (analyse_positions with the evaluator's own iterations and settings)
and solved in one batch, instead of one search and one solver call per position.
"""
import logging
import os
import random

import torch

from .arena import GAMES, game_of_env
from .solve import DEFAULT_MAX_NODES, ILLEGAL, perfect_report, solve_to_end


def parse_position(text, n_actions):
    """A position line -> its moves, 0-based: the first space-separated field is the move string in 1-based
    column digits (the reference's _text_to_board).  An empty field is the empty board."""
    field = text.split(" ")[0].strip() if text.strip() else ""
    moves = []
    for ch in field:
        if not ch.isdigit() or not 1 <= int(ch) <= n_actions:
            raise ValueError(f"position {text!r}: {ch!r} is not a column digit in 1 .. {n_actions}")
        moves.append(int(ch) - 1)
    return moves


def read_positions(positions, n_actions):
    """A list of position lines (or of 0-based move lists), or the path of a file with one position per line."""
    if isinstance(positions, (str, os.PathLike)):
        with open(positions) as f:
            positions = [line.rstrip("\n") for line in f if line.strip()]
    out = []
    for p in positions:
        out.append(parse_position(p, n_actions) if isinstance(p, str) else [int(a) for a in p])
    return out


class PerfectEvaluator:
    """PerfectEvaluator(evaluator, positions): evaluator is an MCTreeSearch (its network, iterations and search
    settings are used); positions a list or a file of move strings.  max_nodes: the solver's budget per position;
    positions it does not solve within it are reported and never counted.  seed: of the sampling (None: the
    global random module, as the reference)."""

    def __init__(self, evaluator, positions, max_nodes=DEFAULT_MAX_NODES, seed=None):
        self.evaluator = evaluator
        self.game = getattr(evaluator, "game", None) or game_of_env(evaluator.env)
        self.n_actions = GAMES[self.game][3]
        self.pos_list = read_positions(positions, self.n_actions)
        self.max_nodes = max_nodes
        self.rng = random.Random(seed) if seed is not None else random
        self.table = None
        self.last = None  # the tensors of the last test(): per base_network value

    # ------------------------------------------------------------------ the evaluator's moves
    def _search_kwargs(self):
        e = self.evaluator
        arena = getattr(e, "_arena", None)
        return dict(iterations=int(e.iterations), search_threads=int(getattr(arena, "search_threads", 1)),
                    strong_play=bool(getattr(e, "strong_play", False)), alpha=float(getattr(e, "alpha", 1.0)),
                    cpuct=float(getattr(e, "cpuct", 4.0)), x_noise=float(getattr(e, "x_noise", 0.25)),
                    seed=int(getattr(e, "seed", 0) or 0), device=getattr(e, "device", None))

    def choose(self, games, base_network=False, solved=None):
        """The evaluator's move for each position: the search's most visited child, or with base_network the
        argmax of the raw network policy on the board seen by the side to move."""
        from .mcts import analyse_positions

        if not base_network:
            return analyse_positions(self.game, self.evaluator.network, games, **self._search_kwargs())["action"]
        boards = solved["boards"].long() * solved["players"].long().reshape(-1, 1, 1)  # own stones = +1
        net = self.evaluator.network
        with torch.no_grad():
            probs = net.forward(boards)[0]
        return probs.reshape(len(games), -1).argmax(dim=1)

    def solve(self, games):
        """solve_to_end on the positions, with their boards and players."""
        from .solve import SolveTable, positions_to_boards

        boards, players = positions_to_boards(self.game, games)
        dev = getattr(self.evaluator, "device", None)
        if self.table is None:
            self.table = SolveTable(self.game, device=dev)
        out = solve_to_end(self.game, boards=boards, players=players, max_nodes=self.max_nodes, table=self.table)
        out["boards"] = torch.as_tensor(boards).to(out["score"].device)
        out["players"] = torch.as_tensor(players).to(out["score"].device)
        return out

    # ------------------------------------------------------------------ the reference's surface
    def test(self, num_pos=100, base_network=False, weak=False):
        """Sample num_pos positions; count the evaluator's correct moves (weak: moves that keep the win, draw or
        loss; else moves with the best code) over the positions the solver solved.  One line per base_network
        value as the reference: with base_network both the raw network (True) and the search (False).  Returns
        the list of {"base_network", "total", "n_solved", "n_unsolved", "line"}."""
        games = self.rng.sample(self.pos_list, num_pos)
        solved = self.solve(games)
        self.last = {}
        results = []
        for compare_val in ([True, False] if base_network else [False]):
            action = self.choose(games, base_network=compare_val, solved=solved)
            rep = self.report(solved["score"], action, weak)
            total = rep["n_weak"] if weak else rep["n_strong"]
            line = f"{total} correct moves out of {rep['n_solved']}: base_network = {compare_val}"
            if rep["n_unsolved"]:
                line += f" ({rep['n_unsolved']} positions not solved within {self.max_nodes} nodes, not counted)"
            logging.info(line)
            print(line)
            self.last[compare_val] = dict(games=games, action=action, score=solved["score"], report=rep)
            results.append(dict(base_network=compare_val, total=total, n_solved=rep["n_solved"],
                                n_unsolved=rep["n_unsolved"], line=line))
        return results

    @staticmethod
    def report(score, action, weak=False):
        """perfect_report with an illegal choice (the raw network's argmax may be one) counted as incorrect."""
        action = torch.as_tensor(action).to(score.device, torch.int64).reshape(-1)
        illegal = score.long().gather(1, action.reshape(-1, 1)).reshape(-1) == ILLEGAL if len(action) else action > 0
        legal_any = (score != ILLEGAL).to(torch.int64).argmax(dim=1) if len(action) else action
        rep = perfect_report(score, torch.where(illegal, legal_any, action))
        for k in ("strong", "weak"):
            rep[k] = rep[k] & ~illegal
            rep["n_" + k] = int(rep[k].sum())
        return rep

    def compare(self, moves, base_network=False, weak=False):
        """One position (a move string or a 0-based move list): 1 if the evaluator's move is correct, else 0
        (0 too where the solver gave up)."""
        games = read_positions([moves], self.n_actions)
        solved = self.solve(games)
        rep = self.report(solved["score"], self.choose(games, base_network=base_network, solved=solved), weak)
        return int(rep["n_weak"] if weak else rep["n_strong"])
