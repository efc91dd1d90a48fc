"""Exact-arithmetic nets, operands and fp64 references for the MFMA kernels (host only).

The fused trunk, the linear heads and the trainer's 3x3 convolutions share one numeric contract: fp16 / bf16
operands, products accumulated in fp32, one round-to-nearest-even per stored output.  With integer-valued
operands (the heads: a power-of-two grid) whose |products| sum to less than 2^24 per output, every fp32
partial sum is exact whatever the order, so the kernel's output is determined: RNE_dtype of the fp64 result.
tests/test_exact_nets.py checks those preconditions on the host; tests/test_gpu_exact_kernels.py compares the
kernels with `torch.equal`.

Nothing here touches a GPU or loads the native library: the package's modules are imported inside the functions.
"""
import functools
import math

import torch
from torch.nn import functional as F

F64 = torch.float64
LIMIT = float(2 ** 24)          # fp32 holds every integer below it
LOGIT_STEP, LOGIT_MAX = 1.0 / 8, 4.0
Z_STEP, Z_MAX = 1.0 / 64, 2.0
PROB_RTOL = 1e-3                # heads: probabilities, relative, against the fp64 softmax
VALUE_ATOL = 1e-4               # heads: value, absolute, against the fp64 tanh
CALIB_BOARDS = 65               # the heads are scaled on exact_boards(W, H, 65, BOARD_SEED)
BOARD_SEED = 11
BN_EPS = 1e-300                 # torch refuses eps = 0; 1 + 1e-300 == 1 in float64, so BatchNorm scales by exactly 1


# ----------------------------------------------------------------------------- boards
def exact_boards(W, H, n, seed=BOARD_SEED):
    """[n, W, H] boards in {-1, 0, 1}, all different: a full board, a random board, the empty board, a single
    stone in a corner, a random board, a single stone in each other corner, then random boards (batches of at
    least 8 hold all of them).  A longer batch of the same seed starts with the shorter one."""
    g = torch.Generator().manual_seed(seed)

    def corner(x, y, s):
        b = torch.zeros(W, H, dtype=torch.int64)
        b[x, y] = s
        return b

    full = torch.randint(0, 2, (W, H), generator=g) * 2 - 1
    fixed = {0: full, 2: torch.zeros(W, H, dtype=torch.int64), 3: corner(0, 0, 1), 5: corner(W - 1, H - 1, -1),
             6: corner(0, H - 1, -1), 7: corner(W - 1, 0, 1)}
    seen = {tuple(b.reshape(-1).tolist()) for b in fixed.values()}
    boards = []
    while len(boards) < n:
        if len(boards) in fixed:
            boards.append(fixed[len(boards)])
            continue
        fill = 0.2 + 0.6 * torch.rand((), generator=g).item()
        b = (torch.rand(W, H, generator=g) < fill).long() * (torch.randint(0, 2, (W, H), generator=g) * 2 - 1)
        key = tuple(b.reshape(-1).tolist())
        if key not in seen:
            seen.add(key)
            boards.append(b)
    return torch.stack(boards)


def exact_planes(W, H, n, seed=BOARD_SEED):
    """float [n, 3, W, H] one-hot (empty, own, enemy) planes of exact_boards."""
    from self_play_reinforcement_learning_amd.modules import planes_from_boards

    return planes_from_boards(exact_boards(W, H, n, seed), W, H)


# ----------------------------------------------------------------------------- nets
def _sparse_signs(rows, cols, per_row, g, negative_only=False):
    """[rows, cols] with `per_row` entries of +-1 per row (the rest 0), without a Python loop over rows."""
    idx = torch.rand(rows, cols, generator=g).topk(per_row, dim=1).indices
    sign = -torch.ones(rows, per_row) if negative_only else (torch.randint(0, 2, (rows, per_row), generator=g) * 2.0 - 1)
    return torch.zeros(rows, cols).scatter_(1, idx, sign)


def _set_conv(conv, bn, g, per_row=4, beta=(-2, 1), negative_only=False):
    cout = conv.weight.shape[0]
    conv.weight.copy_(_sparse_signs(cout, conv.weight[0].numel(), per_row, g, negative_only).view_as(conv.weight))
    conv.bias.zero_()
    bn.eps = BN_EPS  # identity statistics: the folded weights and biases are the integers themselves
    bn.running_mean.zero_()
    bn.running_var.fill_(1.0)
    bn.weight.fill_(1.0)
    if beta is None:
        bn.bias.zero_()
    else:
        bn.bias.copy_(torch.randint(beta[0], beta[1] + 1, (cout,), generator=g).float())


KINDS = ("small", "round", "deep")


@torch.no_grad()
def exact_tower(W, H, A, blocks, ff, seed, kind, heads=True):
    """A ResidualTower (eval, CPU, fp32 parameters) whose eval forward is integer arithmetic: BatchNorm the
    identity plus an integer shift in [-2, 1], four weights of +-1 per output channel of every conv, conv bias 0.

    kind: "small" = every layer at most 256 (exact in fp16 and bf16); "round" = five weights per output channel
    of the block convs, so that 5 blocks reach layers above 256 and below 2048 (bf16 has to round them, fp16
    does not); "deep" = each block's conv2 keeps one weight of -1 per channel and bn2 shifts by 0, so
    x <- relu(x - something >= 0) cannot grow however many blocks follow; its stem shifts by [2, 12] and the
    blocks' conv1 by [-8, -3], so that the activations start high and sink slowly: every one of 20 blocks still
    changes them (with the [-2, 1] shifts the net reaches a fixed point after a dozen blocks and the later convs
    could be dropped unnoticed).  tests/test_exact_nets.py asserts the ranges for the depths the GPU tests use.

    heads: the linear heads get sparse weights of +-1/8, scaled on exact_planes(W, H, 65) so that the fp64
    logits are multiples of 1/8 in [-4, 4] and the value pre-activation a multiple of 1/64 in [-2, 2]
    (False: they keep their default initialisation; the trunk does not read them)."""
    from self_play_reinforcement_learning_amd.modules import ResidualTower

    assert kind in KINDS, kind
    net = ResidualTower(W, H, A, num_blocks=blocks, filter_factor=ff).eval()
    g = torch.Generator().manual_seed(seed)
    _set_conv(net.conv1, net.bn1, g, beta=(2, 12) if kind == "deep" else (-2, 1))
    per_row = 5 if kind == "round" else 4
    for blk in net.residual_blocks:
        _set_conv(blk.conv1, blk.bn1, g, per_row=per_row, beta=(-8, -3) if kind == "deep" else (-2, 1))
        if kind == "deep":
            _set_conv(blk.conv2, blk.bn2, g, per_row=1, beta=None, negative_only=True)
        else:
            _set_conv(blk.conv2, blk.bn2, g, per_row=per_row)
    _set_conv(net.conv_policy, net.policy_bn, g)
    _set_conv(net.conv_value, net.value_bn, g)
    if heads:
        feats = trunk_reference(net, exact_planes(W, H, CALIB_BOARDS), None, bounds=False)[0]
        _scale_heads(net, feats, g)
    return net


def _nchw_cols(feats_half):
    """[n, cells, ff] features -> [n, ff * cells] in the module's flatten(1) order of [n, ff, W, H]."""
    return feats_half.permute(0, 2, 1).reshape(feats_half.shape[0], -1)


def _quiet_rows(rows, peak, lo, hi, per_row, g):
    """[rows, K] weights of +-1/8 at `per_row` inputs per row whose peak over the scaling boards is in [lo, hi]."""
    cand = ((peak >= lo) & (peak <= hi)).nonzero().reshape(-1)
    if cand.numel() < per_row:
        raise ValueError("no quiet head features for this seed: pick another")
    pick = torch.rand(rows, cand.numel(), generator=g).topk(per_row, dim=1).indices
    sign = torch.randint(0, 2, (rows, per_row), generator=g) * 2.0 - 1
    return torch.zeros(rows, peak.numel()).scatter_(1, cand[pick], sign * LOGIT_STEP)


def _scale_heads(net, feats, g):
    ff = net.filter_factor
    pf, vf = _nchw_cols(feats[..., :ff]), _nchw_cols(feats[..., ff:])
    # policy: 4 inputs that stay within 6 on the scaling boards (|sum| <= 3) + a bias in [-1, 1]
    net.linear_policy.weight.copy_(_quiet_rows(net.action_size, pf.max(0).values, 1, 6, 4, g))
    net.linear_policy.bias.copy_(torch.randint(-8, 9, (net.action_size,), generator=g) * LOGIT_STEP)
    # value: hidden = relu(2 inputs within 8 + a bias in [-1, 1/2]) in steps of 1/8; output weights +-1/8, thinned
    # until |z| <= 2 on the scaling boards
    hid = net.fc_value.weight.shape[0]
    net.fc_value.weight.copy_(_quiet_rows(hid, vf.max(0).values, 1, 8, 2, g))
    net.fc_value.bias.copy_(torch.randint(-8, 5, (hid,), generator=g) * LOGIT_STEP)
    wo = (torch.randint(0, 2, (hid,), generator=g) * 2.0 - 1) * LOGIT_STEP
    net.linear_output.bias.fill_(8 * Z_STEP)
    h = torch.relu(vf @ net.fc_value.weight.double().t() + net.fc_value.bias.double())
    while (h @ wo.double() + 8 * Z_STEP).abs().max() > Z_MAX:
        live = wo.nonzero().reshape(-1)
        if live.numel() < 8:
            raise ValueError("value head cannot be scaled for this seed: pick another")
        wo[live[1::2]] = 0.0
    net.linear_output.weight.copy_(wo.view(1, -1))


# ----------------------------------------------------------------------------- references
def rne(x, dtype):
    """fp64 -> RNE_dtype -> fp64 (dtype None: unrounded).  The values are integers below 2^24, so the fp32 step
    between is exact and the rounding to `dtype` happens once."""
    return x if dtype is None else x.float().to(dtype).double()


def folded_layers(net, dtype):
    """[(w fp64 of the dtype-rounded folded weights, b fp64 of the fp32 bias, role)] in layer order; role in
    "stem", "conv1", "conv2", "head" (the head: policy ff output channels, then value ff)."""
    from self_play_reinforcement_learning_amd.modules import InferenceTower

    fold = InferenceTower._fold
    pairs = [(net.conv1, net.bn1, "stem")]
    for blk in net.residual_blocks:
        pairs += [(blk.conv1, blk.bn1, "conv1"), (blk.conv2, blk.bn2, "conv2")]
    out = []
    for conv, bn, role in pairs:
        w, b = fold(conv, bn)
        out.append((rne(w, dtype), b.float().double(), role))
    wp, bp = fold(net.conv_policy, net.policy_bn)
    wv, bv = fold(net.conv_value, net.value_bn)
    out.append((rne(torch.cat([wp, wv], 0), dtype), torch.cat([bp, bv], 0).float().double(), "head"))
    return out


@torch.no_grad()
def run_layers(layers, x, dtype, start=0, resid=None, bounds=True, keep=None, rejoin=None):
    """The trunk from layer `start` on: x = that layer's input [n, c, W, H] (fp64), resid = the running block's
    input (needed when `start` is a conv2).  Every layer's output is RNE_dtype(relu(acc + bias [+ block input])),
    rounded once, after the residual add (csrc/tower_common.h Ty::add_pk / relu_pk).  keep: a list that receives
    (x, resid) before every layer.  rejoin: such a list of another run; the run ends with x = None as soon as its
    state equals that run's before a later layer (the rest would repeat it).  Returns (head output [n, 2ff, W, H], [max |value| per layer], max sum |products|)."""
    maxes, prod = [], 0.0
    for i in range(start, len(layers)):
        w, b, role = layers[i]
        if keep is not None:
            keep.append((x, resid))
        if rejoin is not None and i > start and torch.equal(x, rejoin[i][0]) and (
                role != "conv2" or torch.equal(resid, rejoin[i][1])):
            return None, maxes, prod
        if role == "conv1":
            resid = x
        pad = 0 if role == "head" else 1
        acc = F.conv2d(x, w, b, padding=pad)
        if bounds:
            prod = max(prod, (F.conv2d(x.abs(), w.abs(), b.abs(), padding=pad)
                              + (resid.abs() if role == "conv2" else 0)).max().item())
        if role == "conv2":
            acc = acc + resid
        x = rne(torch.relu(acc), dtype)
        maxes.append(x.abs().max().item())
    return x, maxes, prod


def feats_of(head_out):
    """[n, 2ff, W, H] -> [n, cells, 2ff]: the layout of HipTowerEvaluator.trunk()."""
    n, c = head_out.shape[:2]
    return head_out.permute(0, 2, 3, 1).reshape(n, -1, c)


@torch.no_grad()
def trunk_reference(net, planes, dtype, bounds=True):
    """fp64 on the CPU: (head features [n, cells, C/2] (policy ff channels, then value ff), every layer's
    max |value|, the max sum of |products| (bias and residual included) into any output)."""
    out, maxes, prod = run_layers(folded_layers(net, dtype), planes.double().cpu(), dtype, bounds=bounds)
    return feats_of(out), maxes, prod


@torch.no_grad()
def module_features(net, planes):
    """The module's own eval forward in float64 up to the head features, through conv_policy / conv_value + BN +
    relu (modules.py ResidualTower.forward_planes), in trunk()'s layout."""
    import copy

    m = copy.deepcopy(net).double().eval()
    x = m.relu(m.bn1(m.conv1(planes.double())))
    x = m.residual_blocks(x)
    p = F.relu(m.policy_bn(m.conv_policy(x)))
    v = F.relu(m.value_bn(m.conv_value(x)))
    return feats_of(torch.cat([p, v], 1))


@torch.no_grad()
def heads_reference(net, feats):
    """fp64 (logits [n, A], probabilities [n, A], value pre-activation z [n], values [n]) of the module's
    linear heads on head features [n, cells, 2ff]."""
    ff = net.filter_factor
    f = feats.double()
    logits = F.linear(_nchw_cols(f[..., :ff]), net.linear_policy.weight.double(), net.linear_policy.bias.double())
    h = torch.relu(F.linear(_nchw_cols(f[..., ff:]), net.fc_value.weight.double(), net.fc_value.bias.double()))
    z = F.linear(h, net.linear_output.weight.double(), net.linear_output.bias.double()).reshape(-1)
    return logits, torch.softmax(logits, 1), z, torch.tanh(z)


def conv_case(W, H, cin, cout, n, seed):
    """Integer operands of y = conv3x3(x, w) + b and its gradients for the output gradient gy, with their fp64
    reference: dict(x, w, b, gy, y, dx, dw, db), all float64 on the CPU."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-3, 4, (n, cin, W, H), generator=g).double().requires_grad_(True)
    w = torch.randint(-2, 3, (cout, cin, 3, 3), generator=g).double().requires_grad_(True)
    b = torch.randint(-4, 5, (cout,), generator=g).double().requires_grad_(True)
    gy = torch.randint(-3, 4, (n, cout, W, H), generator=g).double()
    y = F.conv2d(x, w, b, padding=1)
    y.backward(gy)
    y0 = F.conv2d(x.detach(), w.detach(), None, padding=1)
    return dict(x=x.detach(), w=w.detach(), b=b.detach(), gy=gy, y=y.detach(), y_nobias=y0, dx=x.grad, dw=w.grad,
                db=b.grad)


# ----------------------------------------------------------------------------- the cases of the GPU tests
GAMES = {(7, 6): 7, (3, 3): 9, (6, 5): 6, (8, 7): 8}  # board -> actions
# boards per full tile of the fused trunk (csrc/tower.hip, tower_boards.hip): the host-count batches are
# 2 x BOARDS + 1 boards, every board slot of a tile plus a partly empty tile
TILE_BOARDS = {(7, 6, 128): 6, (7, 6, 256): 6, (3, 3, 128): 28, (3, 3, 256): 14, (6, 5, 128): 8, (6, 5, 256): 4,
               (8, 7, 128): 4, (8, 7, 256): 2}


def _case(W, H, ff, blocks, kind, seed=0, heads=False):
    return dict(W=W, H=H, A=GAMES[(W, H)], blocks=blocks, ff=ff, seed=seed, kind=kind, heads=heads,
                n=2 * TILE_BOARDS[(W, H, 4 * ff)] + 1)


def case_id(c):
    return f"{c['W']}x{c['H']}-c{4 * c['ff']}-b{c['blocks']}-{c['kind']}"


TRUNK_CASES = (
    [_case(7, 6, ff, d, "small", heads=(d == 3)) for ff in (32, 64) for d in (1, 2, 3)]  # both buffer parities
    + [_case(7, 6, ff, 5, "round") for ff in (32, 64)]
    + [_case(7, 6, ff, 20, "deep") for ff in (32, 64)]
    + [_case(3, 3, ff, 3, "small", heads=(ff == 32)) for ff in (32, 64)]
    + [_case(W, H, ff, 3, "small") for (W, H) in ((6, 5), (8, 7)) for ff in (32, 64)]
    + [_case(8, 7, 32, 5, "round")]
)
# the nets the heads tests run (FF = 32 and 64 on 7x6, A = 9 on 3x3): the trunk cases built with scaled heads
HEADS_CASES = [c for c in TRUNK_CASES if c["heads"]]
HEADS_N = (1, 31, 32, 33, 65)
# device-count path: row counts that select each tail kind of k_tower_dyn when the launch is packed (one
# "CU": whole full tiles, then the smallest tile that covers the rest), and one count for the one-kind sets
DEV_COUNTS = [((3, 3, 32), (28 + 14, 28 + 21, 28 + 27)), ((6, 5, 32), (8 + 4, 8 + 6, 8 + 7)), ((8, 7, 32), (4 + 2, 4 + 3)),
              ((7, 6, 32), (6 + 5,)), ((7, 6, 64), (6 + 2,)), ((3, 3, 64), (14 + 9,)), ((6, 5, 64), (4 + 3,)),
              ((8, 7, 64), (2 + 1,))]

CONV_SEED = 5
CONV_SHAPES = [  # (W, H, cin, cout, n): every pair with a partial 8-board slice and with 6x5
    (7, 6, 128, 128, 5), (7, 6, 128, 256, 9), (7, 6, 256, 128, 17), (7, 6, 256, 256, 1), (7, 6, 128, 128, 8),
    (6, 5, 128, 128, 9), (6, 5, 128, 256, 5), (6, 5, 256, 128, 1), (6, 5, 256, 256, 17),
    (3, 3, 128, 256, 8), (3, 3, 256, 128, 9), (3, 3, 256, 256, 5), (3, 3, 128, 128, 17),
]


@functools.lru_cache(maxsize=None)
def _net_cached(key):
    W, H, A, blocks, ff, seed, kind, heads = key
    return exact_tower(W, H, A, blocks, ff, seed, kind, heads=heads)


def case_net(c):
    """The case's net, built once per process (treat it as read-only)."""
    return _net_cached((c["W"], c["H"], c["A"], c["blocks"], c["ff"], c["seed"], c["kind"], c["heads"]))


@functools.lru_cache(maxsize=None)
def _ref_cached(key, n, dtype, bounds):
    net = _net_cached(key)
    return trunk_reference(net, exact_planes(key[0], key[1], n), dtype, bounds=bounds)


def case_reference(c, dtype, n=None, bounds=False):
    """trunk_reference of the case's net on its first n boards (default: the case's batch), computed once per
    process and shared by the tests (read-only)."""
    key = (c["W"], c["H"], c["A"], c["blocks"], c["ff"], c["seed"], c["kind"], c["heads"])
    return _ref_cached(key, c["n"] if n is None else n, dtype, bounds)


def tanh_slope(z):
    return 1.0 - math.tanh(z) ** 2
