"""GPU: the fused trunk, the linear heads and the trainer's 3x3 convolutions against fp64, bit for bit.

All three kernel groups take fp16 / bf16 operands, accumulate the products in fp32 and round each stored output
once, to nearest even.  On the integer-valued nets and operands of tests/exact_helpers.py every fp32 partial sum
is exact in any order, so the output is determined -- RNE_dtype of the fp64 result -- and the comparison is
`torch.equal`: a wrong tap on one edge tile, two swapped channels, a board slot reading a neighbour's row,
truncation instead of rounding ("round" nets: bf16 has to round integers above 256) or a residual rounded twice
all change bits.  tests/test_exact_nets.py asserts the preconditions on the host.

The heads end in __expf / tanhf, so their outputs carry the tolerances derived in the issue: probabilities
relative 1e-3 against the fp64 softmax (one logit step of 1/8 moves a probability by more than 10 %), values
absolute 1e-4 (one step of 1/64 in the pre-activation moves tanh by at least 1e-3).
"""
import pytest
import torch

from tests import exact_helpers as eh

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
SENTINEL = -3.0  # no feature (relu), probability or value (tanh) can be -3


def _hip(c, dtype):
    from self_play_reinforcement_learning_amd.evaluator import HipTowerEvaluator

    return HipTowerEvaluator(eh.case_net(c), device=torch.device("cuda"), dtype=dtype)


def _nhwc(W, H, n):
    """bf16 [n, W, H, 3] contiguous planes on the device (what HipTowerEvaluator.trunk reads)."""
    return eh.exact_planes(W, H, n).permute(0, 2, 3, 1).contiguous().to(torch.bfloat16).cuda()


def _assert_features(got, ref, c, what):
    got = got.double().cpu()
    if torch.equal(got, ref):
        return
    bad = (got != ref).nonzero()
    first = [f"(board {b}, cell {p}, channel {ch}): kernel {got[b, p, ch].item()} reference {ref[b, p, ch].item()}"
             for b, p, ch in bad[:8].tolist()]
    boards = sorted(set(bad[:, 0].tolist()))
    raise AssertionError(f"{what}, {eh.case_id(c)} ({2 * c['blocks'] + 2} layers deep): {bad.shape[0]} of {ref.numel()} "
                         f"features differ, boards {boards}; first " + "; ".join(first))


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("c", eh.TRUNK_CASES, ids=[eh.case_id(c) for c in eh.TRUNK_CASES])
def test_trunk_host_count(c, dtype):
    """HipTowerEvaluator.trunk() on 2 x BOARDS + 1 different boards (every board slot of a tile and a partly
    empty tile) equals RNE_dtype of the fp64 trunk."""
    ref = eh.case_reference(c, dtype)[0]
    got = _hip(c, dtype).trunk(_nhwc(c["W"], c["H"], c["n"]))
    assert got.shape == ref.shape and got.dtype == dtype
    _assert_features(got, ref, c, "host-count trunk")


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("key,counts", eh.DEV_COUNTS, ids=[f"{k[0]}x{k[1]}-c{4 * k[2]}" for k, _ in eh.DEV_COUNTS])
def test_trunk_device_count(key, counts, dtype):
    """tower_dev (k_tower_dyn, packed launch: whole full tiles, then the smallest tile kind that covers the
    rest) at row counts that select each tail kind: the live rows equal the fp64 trunk, the rows past the count
    keep their sentinel."""
    W, H, ff = key
    c = next(c for c in eh.TRUNK_CASES if (c["W"], c["H"], c["ff"], c["blocks"], c["kind"]) == (W, H, ff, 3, "small"))
    hip = _hip(c, dtype)
    hip.concurrent = True
    boards = eh.TILE_BOARDS[(W, H, 4 * ff)]
    for count in counts:
        max_rows = count + boards + 3
        planes = _nhwc(W, H, max_rows)
        ref = eh.case_reference(c, dtype, n=count)[0]
        hip._dev_bufs = None
        hip.reserve(max_rows, planes.device)
        feats = hip._dev_bufs[0]
        assert feats.shape[0] == max_rows
        feats.fill_(SENTINEL)
        hip.tower_dev(planes, torch.tensor([count], dtype=torch.int32, device="cuda"), max_rows)
        torch.cuda.synchronize()
        _assert_features(feats[:count], ref, c, f"device-count trunk, {count} rows")
        assert bool((feats[count:] == SENTINEL).all()), f"{count} rows: rows past the count were written"


def _assert_heads(p, v, net, feats_ref, what):
    logits, probs, z, values = eh.heads_reference(net, feats_ref)
    p, v = p.double().cpu(), v.double().cpu().reshape(-1)
    assert p.shape == probs.shape and v.shape == values.shape, what
    rel = ((p - probs).abs() / probs).max().item()
    err = (v - values).abs().max().item()
    print(f"{what}: max relative probability error {rel:.3e}, max value error {err:.3e}")
    assert rel <= eh.PROB_RTOL, (what, rel)
    assert err <= eh.VALUE_ATOL, (what, err)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("c", eh.HEADS_CASES, ids=[eh.case_id(c) for c in eh.HEADS_CASES])
def test_heads(c, dtype):
    """hip(x) (trunk + k_heads_co) for n = 1, 31, 32, 33, 65 against the fp64 softmax / tanh of the fp64 logits
    (multiples of 1/8) and pre-activations (multiples of 1/64), then the heads_dev path with a count below the
    buffer rows: rows past the ragged tail keep their sentinel."""
    net = eh.case_net(c)
    hip = _hip(c, dtype)
    W, H = c["W"], c["H"]
    top = max(eh.HEADS_N)
    planes = _nhwc(W, H, top + 7)
    ref = eh.case_reference(c, dtype, n=top)[0]
    for n in eh.HEADS_N:
        p, v = hip(planes[:n].permute(0, 3, 1, 2))
        _assert_heads(p, v, net, ref[:n], f"{eh.case_id(c)} n={n}")
    for count in (33, top):
        rows = top + 7
        hip._dev_bufs = None
        hip.reserve(rows, planes.device)
        _, probs, values = hip._dev_bufs
        probs.fill_(SENTINEL)
        values.fill_(SENTINEL)
        cnt = torch.tensor([count], dtype=torch.int32, device="cuda")
        hip.tower_dev(planes, cnt, rows)
        pd, vd = hip.heads_dev(cnt, rows)
        torch.cuda.synchronize()
        assert pd.shape[0] == rows and vd.shape[0] == rows
        _assert_heads(pd[:count], vd[:count], net, ref[:count], f"{eh.case_id(c)} heads_dev count={count}")
        assert bool((pd[count:] == SENTINEL).all()) and bool((vd[count:] == SENTINEL).all()), count


def _conv_run(k, bias=True, channels_last=False):
    from self_play_reinforcement_learning_amd.trainconv import Conv3x3, supported

    W, H = k["x"].shape[2:]
    assert supported(W, H, k["w"].shape[1], k["w"].shape[0])
    x = k["x"].half().cuda()
    if channels_last:
        x = x.contiguous(memory_format=torch.channels_last)
        assert not x.is_contiguous()
    x.requires_grad_(True)
    w = k["w"].float().cuda().requires_grad_(True)  # the fp32 parameters, as the trainer holds them
    b = k["b"].float().cuda().requires_grad_(True) if bias else None
    with torch.autocast("cuda", dtype=torch.float16):
        y = Conv3x3.apply(x, w, b)
    y.backward(k["gy"].half().cuda())
    torch.cuda.synchronize()
    return y.detach(), x.grad, w.grad, None if b is None else b.grad


def _assert_conv(got, ref, dtype, what):
    assert got.dtype == dtype and got.shape == ref.shape, what
    want = ref.half().to(dtype)  # the fp64 reference rounded to fp16 (dw, db: handed back as fp32)
    if not torch.equal(got.cpu(), want):
        bad = (got.cpu() != want).nonzero()
        raise AssertionError(f"{what}: {bad.shape[0]} of {want.numel()} differ; first at {bad[:4].tolist()}: kernel "
                             f"{[got.cpu()[tuple(i)].item() for i in bad[:4]]} reference {[want[tuple(i)].item() for i in bad[:4]]}")


@pytest.mark.parametrize("W,H,cin,cout,n", eh.CONV_SHAPES)
def test_trainconv(W, H, cin, cout, n):
    """Conv3x3.apply under fp16 autocast on integer operands: y, dx (fp16) and dw, db (fp32 of the fp16 sums)
    equal the fp64 conv2d reference, for cin != cout as well (the packed backward weights' row stride is cout,
    the forward's cin) and for whole and partial 8-board slices of the weight gradient."""
    k = eh.conv_case(W, H, cin, cout, n, eh.CONV_SEED)
    y, dx, dw, db = _conv_run(k)
    what = f"{W}x{H} {cin}->{cout} n={n}"
    _assert_conv(y, k["y"], torch.float16, what + " y")
    _assert_conv(dx, k["dx"], torch.float16, what + " dx")
    _assert_conv(dw, k["dw"], torch.float32, what + " dw")
    _assert_conv(db, k["db"], torch.float32, what + " db")


def test_trainconv_variants():
    """bias=None, a channels_last (non-contiguous) x, and weight_grad(..., bias_grad=False)."""
    from self_play_reinforcement_learning_amd.trainconv import weight_grad

    W, H, cin, cout, n = 7, 6, 128, 256, 9
    k = eh.conv_case(W, H, cin, cout, n, eh.CONV_SEED)
    y, dx, dw, db = _conv_run(k, bias=False)
    assert db is None
    _assert_conv(y, k["y_nobias"], torch.float16, "bias=None y")
    _assert_conv(dx, k["dx"], torch.float16, "bias=None dx")
    _assert_conv(dw, k["dw"], torch.float32, "bias=None dw")
    y, dx, dw, db = _conv_run(k, channels_last=True)
    _assert_conv(y, k["y"], torch.float16, "channels_last y")
    _assert_conv(dx, k["dx"], torch.float16, "channels_last dx")
    _assert_conv(dw, k["dw"], torch.float32, "channels_last dw")
    _assert_conv(db, k["db"], torch.float32, "channels_last db")
    dw, db = weight_grad(k["x"].half().cuda(), k["gy"].half().cuda(), bias_grad=False)
    torch.cuda.synchronize()
    assert db is None
    _assert_conv(dw, k["dw"], torch.float32, "bias_grad=False dw")
