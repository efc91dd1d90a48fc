"""The boards' left-right mirror symmetry: helpers, the canonical form of a network input, SymmetricNet.

Every board the arena plays is left-right symmetric.  M maps cell (x, y) to (W-1-x, y): a flip of axis 0 of the
[W][H] boards.  The action map m is a -> W-1-a on the gravity boards and a = x*H + y -> (W-1-x)*H + y on tictactoe;
both are involutions.

The canonical form of a leaf's network input (own, opp) -- the mover's and the opponent's stones -- is the mirror
image iff (M own, M opp) < (own, opp), compared as pairs of unsigned 64-bit bitboards of csrc/board.h's layout (cell
(x, y) = bit x*(H+1) + y), own first.  A self-symmetric position is never flipped.  With symmetry="mirror" an arena
evaluates canonical inputs only (Arena.set_symmetry; include/spmcts.h spmcts_set_symmetry) and so searches

    f(x) = g(x)                          where x is not flipped
    f(x) = (m(g(Mx).probs), g(Mx).value) otherwise

which SymmetricNet states for any `net(state, player)` callable of the reference's protocol.  f(Mx) = m(f(x)) bit for
bit for every position that is not self-symmetric.
"""
import ctypes

import numpy as np

# name -> (width, height, gravity): the boards of arena.GAMES (kept here so that this module needs neither torch
# nor the library until library_canonical is called)
_BOARDS = {"connect4": (7, 6, True), "connect4_6_5": (6, 5, True), "connect4_8_7": (8, 7, True),
           "tictactoe": (3, 3, False)}


def _board(game):
    try:
        return _BOARDS[game]
    except KeyError:
        raise ValueError(f"unknown game {game!r} (one of {', '.join(_BOARDS)})") from None


def _is_tensor(x):
    return type(x).__module__.startswith("torch")


def mirror_boards(game, boards):
    """M of boards [..., W, H] (numpy array or torch tensor): the flip of the W axis."""
    W, H, _ = _board(game)
    if tuple(boards.shape[-2:]) != (W, H):
        raise ValueError(f"{game} boards are [..., {W}, {H}], got {tuple(boards.shape)}")
    if _is_tensor(boards):
        return boards.flip(-2)
    return np.flip(np.asarray(boards), axis=-2).copy()


def mirror_actions(game, like=None):
    """The permutation m as an index array: m[a] is the mirror image of action a (int64 numpy array; a torch
    tensor on `like`'s device when `like` is a tensor)."""
    W, H, gravity = _board(game)
    if gravity:
        m = np.arange(W - 1, -1, -1, dtype=np.int64)
    else:
        a = np.arange(W * H, dtype=np.int64)
        m = (W - 1 - a // H) * H + a % H
    if like is not None and _is_tensor(like):
        import torch

        return torch.as_tensor(m, device=like.device)
    return m


def mirror_probs(game, probs):
    """Action-indexed rows [..., A] seen from the mirror image: out[..., a] = probs[..., m(a)]."""
    m = mirror_actions(game, like=probs)
    if probs.shape[-1] != len(m):
        raise ValueError(f"{game} has {len(m)} actions, got rows of {probs.shape[-1]}")
    if _is_tensor(probs):
        return probs[..., m]
    return np.asarray(probs)[..., m]


def mirror_moves(game, moves):
    """A move list (an opening), or a list of them, played on the mirror image: every action a becomes m(a)."""
    m = mirror_actions(game)
    if len(moves) and isinstance(moves[0], (list, tuple, np.ndarray)):
        return [mirror_moves(game, s) for s in moves]
    return [int(m[int(a)]) for a in moves]


def _masks(game, planes):
    """uint64 bitboards (csrc/board.h's layout) of boolean planes [..., W, H]."""
    W, H, _ = _board(game)
    w = (np.uint64(1) << (np.arange(W, dtype=np.uint64)[:, None] * np.uint64(H + 1)
                          + np.arange(H, dtype=np.uint64)[None, :]))
    return (planes.astype(np.uint64) * w).sum(axis=(-2, -1), dtype=np.uint64)


def canonical(game, boards, players):
    """The rule, in numpy: boards int [..., W, H] with stones +1 / -1, players [...] (+1 / -1, the side to move)
    -> (canon int8 [..., W, H] with own = +1 and opp = -1 in canonical orientation, flipped bool [...])."""
    b = np.asarray(boards)
    p = np.asarray(players).reshape(b.shape[:-2])
    x = (b * p[..., None, None]).astype(np.int8)
    mx = np.flip(x, axis=-2)
    own, opp = _masks(game, x == 1), _masks(game, x == -1)
    mown, mopp = _masks(game, mx == 1), _masks(game, mx == -1)
    flipped = (mown < own) | ((mown == own) & (mopp < opp))
    return np.where(flipped[..., None, None], mx, x).astype(np.int8), flipped


def library_canonical(game, boards, players):
    """canonical() by the library's host twin of the kernels' rule (spmcts_canonical_host; no GPU)."""
    from . import _lib
    from .arena import GAMES

    gid, W, H, _ = GAMES[game]
    b = np.ascontiguousarray(np.asarray(boards, dtype=np.int8))
    lead = b.shape[:-2]
    p = np.asarray(players).reshape(lead)
    flat = b.reshape(-1, W, H)
    canon = np.zeros_like(flat)
    flipped = np.zeros(len(flat), dtype=bool)
    f = ctypes.c_int32()
    for i, pl in enumerate(p.reshape(-1)):
        src = np.ascontiguousarray(flat[i])
        _lib.call("spmcts_canonical_host", gid, W, H, src.ctypes.data_as(ctypes.c_void_p), int(pl),
                  canon[i].ctypes.data_as(ctypes.c_void_p), ctypes.byref(f))
        flipped[i] = bool(f.value)
    return canon.reshape(lead + (W, H)), flipped.reshape(lead)


class SymmetricNet:
    """f of a `net(state, player) -> (probs, value)` callable of the reference's protocol (the function an arena
    with symmetry="mirror" searches): the net sees the canonical orientation of every position, and the probs of a
    flipped one come back through m.  A model can so be used outside the arena with the function it was searched
    with."""

    def __init__(self, net, game):
        self.net, self.game = net, game
        self._m = mirror_actions(game)

    def __call__(self, state, player=1):
        s = np.asarray(state)
        _, flipped = canonical(self.game, s, player)
        if not bool(flipped):
            return self.net(state, player)
        probs, value = self.net(np.flip(s, axis=-2).copy(), player)
        if _is_tensor(probs):
            return probs[..., mirror_actions(self.game, like=probs)], value
        if isinstance(probs, np.ndarray):
            return probs[..., self._m], value
        return [probs[int(a)] for a in self._m], value

    def __getattr__(self, name):  # everything else (salt, n_actions, ...) is the wrapped net's
        if name in ("net", "game", "_m"):
            raise AttributeError(name)
        return getattr(self.net, name)
