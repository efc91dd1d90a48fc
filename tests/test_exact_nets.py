"""Host: the preconditions of tests/test_gpu_exact_kernels.py, for every case it runs.

The GPU tests compare kernels with an fp64 reference by `torch.equal`.  That is only sound if the arithmetic
leaves no room for a tolerance (integer operands, sums of |products| below 2^24), only meaningful if the nets
are not trivial (enough nonzero, distinct head features; every conv, tap and input channel matters), and only
independent if the reference is the module's own forward and not a restatement of the packing code.  Each of
those is asserted here, on the CPU.
"""
import pytest
import torch

from tests import exact_helpers as eh

DTYPES = (torch.float16, torch.bfloat16)
IDS = [eh.case_id(c) for c in eh.TRUNK_CASES]


def _on_grid(t, step=1.0):
    return bool(((t / step) == (t / step).round()).all())


def test_case_list_covers_the_issue():
    """Depths 1-3 on 7x6 (both buffer parities), 5-block "round", 20-block "deep", 3x3, the add-on library's
    6x5 / 8x7, one "round" on another board; each batch 2 x BOARDS + 1 different boards."""
    have = {(c["W"], c["H"], 4 * c["ff"], c["blocks"], c["kind"]) for c in eh.TRUNK_CASES}
    for C in (128, 256):
        for d in (1, 2, 3):
            assert (7, 6, C, d, "small") in have
        assert (7, 6, C, 5, "round") in have and (7, 6, C, 20, "deep") in have
        for W, H in ((3, 3), (6, 5), (8, 7)):
            assert (W, H, C, 3, "small") in have
    assert any(k[:2] != (7, 6) and k[3:] == (5, "round") for k in have)
    for c in eh.TRUNK_CASES:
        b = eh.exact_boards(c["W"], c["H"], c["n"])
        assert len({tuple(x.reshape(-1).tolist()) for x in b}) == c["n"] == 2 * eh.TILE_BOARDS[(c["W"], c["H"], 4 * c["ff"])] + 1
        stones = b.abs().sum((1, 2))
        assert stones[0] == c["W"] * c["H"] and stones[2] == 0 and stones[3] == 1  # full, empty, a corner stone
        assert 0 < stones[1] < c["W"] * c["H"] or c["W"] * c["H"] == 9  # a random board
        if c["n"] >= 8:
            corners = b[[3, 5, 6, 7]][:, [0, 0, -1, -1], [0, -1, 0, -1]].abs()
            assert (stones[[3, 5, 6, 7]] == 1).all() and (corners.sum(0) == 1).all()  # a single stone in each corner
        assert torch.equal(b, eh.exact_boards(c["W"], c["H"], eh.CALIB_BOARDS)[: c["n"]])
        planes = eh.exact_planes(c["W"], c["H"], c["n"])
        assert bool((planes.sum(1) == 1).all()) and set(planes.unique().tolist()) == {0.0, 1.0}


@pytest.mark.parametrize("c", eh.TRUNK_CASES, ids=IDS)
def test_exactness(c):
    """Folded weights, biases and every layer's values are integers; the sum of |products| into any output is
    below 2^24; values are at most 256 ("small": exact in both dtypes), at most 2048 in fp16, below 65504."""
    net = eh.case_net(c)
    for dtype in DTYPES:
        layers = eh.folded_layers(net, dtype)
        unrounded = eh.folded_layers(net, None)
        for (w, b, _), (w0, b0, _) in zip(layers, unrounded):
            assert _on_grid(w) and _on_grid(b) and torch.equal(w, w0) and torch.equal(b, b0)
        keep = []
        out, maxes, prod = eh.run_layers(layers, eh.exact_planes(c["W"], c["H"], c["n"]).double(), dtype, keep=keep)
        assert all(_on_grid(x) for x, _ in keep) and _on_grid(out)
        assert prod < eh.LIMIT
        assert max(maxes) < 65504
        if c["kind"] == "small":
            assert max(maxes) <= 256
        if c["kind"] == "deep":
            assert max(maxes) <= 64  # bounded by the stem's output whatever the depth
        if dtype == torch.float16:
            assert max(maxes) <= 2048
        if c["kind"] == "round":
            assert 256 < max(maxes) < 2048


@pytest.mark.parametrize("c", eh.TRUNK_CASES, ids=IDS)
def test_reference_is_the_modules_forward(c):
    """Where nothing rounds, trunk_reference equals the module's own float64 eval forward (conv + BatchNorm +
    relu of modules.py), so the reference is tied to the module and not to the weight packing."""
    net = eh.case_net(c)
    planes = eh.exact_planes(c["W"], c["H"], c["n"])
    mod = eh.module_features(net, planes)
    assert torch.equal(eh.case_reference(c, None)[0], mod)
    for dtype in DTYPES:
        f, maxes, _ = eh.case_reference(c, dtype, bounds=True)
        assert f.shape == (c["n"], c["W"] * c["H"], 2 * c["ff"])
        if max(maxes) <= (2048 if dtype == torch.float16 else 256):
            assert torch.equal(f, mod)


@pytest.mark.parametrize("c", eh.TRUNK_CASES, ids=IDS)
def test_non_trivial(c):
    """Head features: at least 25 % nonzero and 16 distinct values ("deep": 20 % and 4); "round" in bf16: at
    least 1 % differ from the unrounded result; no two boards share their features."""
    need_nz, need_distinct = (0.20, 4) if c["kind"] == "deep" else (0.25, 16)
    for dtype in DTYPES:
        f = eh.case_reference(c, dtype)[0]
        assert (f != 0).double().mean().item() >= need_nz
        assert f.unique().numel() >= need_distinct
        assert len({tuple(x.reshape(-1).tolist()) for x in f}) == c["n"]
    if c["kind"] == "round":
        f, u = eh.case_reference(c, torch.bfloat16)[0], eh.case_reference(c, None)[0]
        assert (f != u).double().mean().item() >= 0.01
        assert torch.equal(eh.case_reference(c, torch.float16)[0], u)  # fp16 holds every integer up to 2048


def _perturbed(layers, i, w):
    out = list(layers)
    out[i] = (w, layers[i][1], layers[i][2])
    return out


@pytest.mark.parametrize("c", eh.TRUNK_CASES, ids=IDS)
def test_sensitivity(c):
    """For each block conv: zeroing its weights, swapping two taps of one output channel, and swapping two
    input channels 4 apart each change the reference features (a kernel that dropped the conv, read a wrong tap
    or permuted channels within a fragment could not pass).  The channel / taps are the first whose swap changes
    that conv's own output; the change must then reach the head features."""
    net = eh.case_net(c)
    dtype = torch.bfloat16
    layers = eh.folded_layers(net, dtype)
    planes = eh.exact_planes(c["W"], c["H"], min(c["n"], 9)).double()
    keep = []
    base = eh.run_layers(layers, planes, dtype, bounds=False, keep=keep)[0]
    for i, (w, b, role) in enumerate(layers):
        if role not in ("conv1", "conv2"):
            continue
        x, resid = keep[i]

        def changed(w2):
            out = eh.run_layers(_perturbed(layers, i, w2), x, dtype, start=i, resid=resid, bounds=False, rejoin=keep)[0]
            return out is not None and not torch.equal(out, base)

        assert changed(torch.zeros_like(w)), (i, "zeroed")
        flat = w.reshape(w.shape[0], w.shape[1], 9)
        # only an output channel that the next layer reads can matter
        read = (layers[i + 1][0].abs().sum((0, 2, 3)) != 0).tolist()
        cands = [k for k in (flat != 0).nonzero().tolist() if read[k[0]]]
        # two taps of one output channel: a nonzero weight and an empty tap of the same input channel
        for o, ci, t in cands:
            t2 = next(k for k in range(9) if flat[o, ci, k] == 0)
            w2 = flat.clone()
            w2[o, :, [t, t2]] = w2[o, :, [t2, t]]
            if changed(w2.view_as(w)):
                break
        else:
            raise AssertionError((i, "taps"))
        for o, ci, t in cands:
            cj = ci + 4 if ci + 4 < w.shape[1] else ci - 4
            w2 = w.clone()
            w2[:, [ci, cj]] = w2[:, [cj, ci]]
            if changed(w2):
                break
        else:
            raise AssertionError((i, "channels"))


@pytest.mark.parametrize("c", eh.HEADS_CASES, ids=[eh.case_id(c) for c in eh.HEADS_CASES])
def test_heads_on_the_grid(c):
    """The fp64 logits are multiples of 1/8 in [-4, 4] and the value pre-activation z a multiple of 1/64 in
    [-2, 2], in both dtypes, on every batch the GPU test runs; head weights are exact in both dtypes; one grid
    step of z moves tanh by at least 10 x the value tolerance; the heads are not trivial."""
    net = eh.case_net(c)
    for p in (net.linear_policy.weight, net.linear_policy.bias, net.fc_value.weight, net.fc_value.bias,
              net.linear_output.weight):
        assert _on_grid(p.double(), eh.LOGIT_STEP) and p.abs().max() <= 1
        for dtype in DTYPES:
            assert torch.equal(p.to(dtype).float(), p)
    assert _on_grid(net.linear_output.bias.double(), eh.Z_STEP)
    assert {4 * c["ff"] for c in eh.HEADS_CASES if (c["W"], c["H"]) == (7, 6)} == {128, 256}
    assert any(c["A"] == 9 for c in eh.HEADS_CASES)
    for dtype in DTYPES:
        f, maxes, _ = eh.case_reference(c, dtype, n=max(eh.HEADS_N), bounds=True)
        assert max(maxes) <= 256
        logits, probs, z, v = eh.heads_reference(net, f)
        assert _on_grid(logits, eh.LOGIT_STEP) and logits.abs().max() <= eh.LOGIT_MAX
        assert _on_grid(z, eh.Z_STEP) and z.abs().max() <= eh.Z_MAX
        # sums of |products| of the heads: far below 2^24 grid steps, so fp32 partial sums are exact
        assert 256 * 4 / eh.LOGIT_STEP < eh.LIMIT and net.fc_value.weight.shape[0] * 8 / eh.Z_STEP < eh.LIMIT
        assert eh.Z_STEP * eh.tanh_slope(z.abs().max().item()) >= 10 * eh.VALUE_ATOL
        # a logit one grid step off moves a probability by more than 10 %: far above the tolerance
        assert 1 - torch.exp(torch.tensor(-eh.LOGIT_STEP)).item() > 0.1 > 10 * eh.PROB_RTOL
        assert logits.unique().numel() >= 8 and z.unique().numel() >= 8
        assert (logits.max(1).values - logits.min(1).values).min() > 0  # no board has a flat policy
        assert (net.linear_output.weight != 0).sum() >= 32


@pytest.mark.parametrize("W,H,cin,cout,n", eh.CONV_SHAPES)
def test_conv_cases_exact(W, H, cin, cout, n):
    """The trainer-conv operands are integers in the stated ranges and every reference output is an integer of
    at most 2048 (exact in fp16, so the kernel's one rounding changes nothing and `torch.equal` is the check)."""
    k = eh.conv_case(W, H, cin, cout, n, eh.CONV_SEED)
    assert k["x"].abs().max() <= 3 and k["gy"].abs().max() <= 3 and k["w"].abs().max() <= 2 and k["b"].abs().max() <= 4
    for name in ("x", "w", "b", "gy", "y", "y_nobias", "dx", "dw", "db"):
        assert _on_grid(k[name]), name
    for name in ("y", "y_nobias", "dx", "dw", "db"):
        assert k[name].abs().max() <= 2048, name
        assert torch.equal(k[name].half().double(), k[name])
        assert k[name].unique().numel() >= 16
    # sum of |products| per output: at most 9 * max(cin, cout) * 6 (+ 4), or n * cells * 9 for the gradients
    assert max(9 * max(cin, cout) * 6 + 4, n * W * H * 9) < eh.LIMIT


def test_conv_shapes_cover_the_axes():
    pairs = {(128, 128), (128, 256), (256, 128), (256, 256)}
    assert {s[2:4] for s in eh.CONV_SHAPES} == pairs
    assert {s[2:4] for s in eh.CONV_SHAPES if s[:2] == (6, 5)} == pairs
    assert {s[2:4] for s in eh.CONV_SHAPES if s[4] % 8} == pairs  # a partial 8-board slice
    assert {s[:2] for s in eh.CONV_SHAPES} == {(7, 6), (6, 5), (3, 3)}
    assert {s[4] for s in eh.CONV_SHAPES} == {1, 5, 8, 9, 17}
