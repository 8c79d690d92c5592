"""GPU parity tests of the squeeze-and-excitation entry points (csrc/se.hip): stp_se_squeeze, stp_se_excite, stp_se_scale_add,
stp_se_bwd_reduce, stp_se_excite_bwd, stp_se_bwd_apply and their sizing queries stp_se_chunks / stp_se_workspace_bytes, each called
directly and compared with the float64 numpy restatement of tests/_se_reference.py - never with a second run of a kernel.

Conventions of tests/test_ops_rest_gpu.py: inputs are rounded through the storage dtype first, ``dtype`` runs over fp32 / bf16 / fp16
with the fp16 cases routed to libstp_hip_f16.so, outputs are pre-filled with NaN, one case has more work items than the launcher's grid
cap (1024 workgroups) so the item loop takes a second trip, one is ragged (odd N, H != W), one is the smallest map (2 x 2); C runs over
64, 128, 256, 512.  Bounds are that file's: ``tol(ref, dtype)`` for the stored tensors (x, du), ``tol(ref, "fp32")`` for the fp32
vectors and parameter gradients.  The statistics table is held to what tests/test_ops_gpu.py asks of a convolution's fused statistics.
b2 is drawn in +-2 (gates spread over (0.05, 0.95)) and b1 makes some hidden units exactly inactive (the ReLU mask is exercised).
"""
import numpy as np
import pytest
import torch

import _se_reference as R
from test_ops_rest_gpu import BADARG, DEV, DTYPES, bits_equal, dev, f32, host, keep, nans, q, rc, tol  # noqa: F401
from test_ops_rest_gpu import _release_device_temporaries, _storage_build, ops  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

GRID_CAP = 1024
# (N, H, W, C)
CASES = [(8, 2, 2, 512),        # the smallest map: stage 4 of a 64-px input (32 values per channel, see `problem`)
         (2, 16, 16, 64),
         (3, 24, 40, 128),      # ragged: odd N, H != W, pixels not a multiple of the chunk
         (4, 64, 64, 256),      # several chunks per image
         (2, 8, 8, 512),
         (1100, 2, 2, 64)]      # more items than the grid cap: the item loop takes a second trip


def problem(case, dtype, seed=0):
    n, h, w, c = case
    r = c // 16
    rng = np.random.RandomState(seed + c + n)
    u = q(rng.randn(n, h, w, c) + 0.3 * rng.randn(1, 1, 1, c), dtype)
    # Conditioning of the statistics check (relative 1e-5 on mean and rstd from a table of fp32 sums): the mean needs |mean| well above
    # the rounding of the sum, hence per-channel offsets of 1..1.5 on the shortcut; rstd comes from E[x^2] - mean^2, whose relative error is
    # ~ kappa / 2 x 2^-23 with kappa = (mean^2 + var) / var, so kappa must stay below ~80: offsets no larger than that, and at least 32 values
    # per channel so that no channel's sample variance collapses (8 values: var 0.04 at mean -4.4 was seen, kappa 450).
    sc = q(rng.randn(n, h, w, c) + rng.uniform(1, 1.5, size=c) * rng.choice([-1.0, 1.0], size=c), dtype)
    dx = q(rng.randn(n, h, w, c) * 0.05, dtype)
    W1 = rng.uniform(-1, 1, size=(c, r)).astype(np.float32) * np.float32(np.sqrt(6.0 / c) * 4)
    b1 = rng.uniform(-0.3, 0.3, size=r).astype(np.float32)
    b1[::3] = -50.0                                    # hidden units 0, 3, 6, ... are exactly inactive for every image
    W2 = rng.uniform(-1, 1, size=(r, c)).astype(np.float32) * np.float32(np.sqrt(6.0 / r))
    b2 = rng.uniform(-2, 2, size=c).astype(np.float32)
    return u, sc, dx, W1, b1, W2, b2


def forward(ops_, case, dtype, u, sc, W1, b1, W2, b2, stats=True):
    n, h, w, c = case
    r, hw = c // 16, h * w
    chunks = ops_.se_chunks(n, hw, c)
    assert chunks >= 1 and ops_.se_workspace_bytes(n, hw, c) == 4 * n * chunks * c
    ws = nans((n * chunks * c,), "fp32")
    z, hh, s = nans((n, c), "fp32"), nans((n, r), "fp32"), nans((n, c), "fp32")
    x = nans((n, h, w, c), dtype)
    table = nans((2, c, n * chunks), "fp32") if stats else None
    du_, dsc = dev(u, dtype), dev(sc, dtype)
    dW1, db1, dW2, db2 = f32(W1), f32(b1), f32(W2), f32(b2)
    ops_.se_squeeze(du_, n, hw, c, ws)
    ops_.se_excite(ws, n, hw, c, r, dW1, db1, dW2, db2, z, hh, s)
    ops_.se_scale_add(du_, dsc, x, n, hw, c, s, table)
    return dict(ws=ws, z=z, h=hh, s=s, x=x, table=table, u=du_, W1=dW1, W2=dW2, chunks=chunks)


def backward(ops_, case, dtype, fw, dx):
    n, h, w, c = case
    r, hw = c // 16, h * w
    ws = nans((n * fw["chunks"] * c,), "fp32")
    ddx = dev(dx, dtype)
    out = dict(da2=nans((n, c), "fp32"), da1=nans((n, r), "fp32"), dz=nans((n, c), "fp32"), dW1=nans((c, r), "fp32"), db1=nans((r,), "fp32"),
               dW2=nans((r, c), "fp32"), db2=nans((c,), "fp32"), du=nans((n, h, w, c), dtype), ws=ws)
    ops_.se_bwd_reduce(ddx, fw["u"], n, hw, c, ws)
    ops_.se_excite_bwd(ws, n, hw, c, r, fw["W1"], fw["W2"], fw["z"], fw["h"], fw["s"], out["da2"], out["da1"], out["dz"], out["dW1"],
                       out["db1"], out["dW2"], out["db2"])
    ops_.se_bwd_apply(ddx, out["du"], n, hw, c, fw["s"], out["dz"])
    return out


def close(got, ref, bound, what):
    got = (host(got) if isinstance(got, torch.Tensor) else np.asarray(got)).astype(np.float64).reshape(ref.shape)
    assert not np.isnan(got).any(), "%s: an element nobody wrote" % what
    err = float(np.abs(got - ref).max())
    print("%s: max err %.3g, bound %.3g" % (what, err, bound))
    assert err <= bound, "%s: max err %.3g > %.3g" % (what, err, bound)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", CASES, ids=lambda c: "%dx%dx%dx%d" % c)
def test_se_forward_matches_float64(ops, case, dtype):
    n, h, w, c = case
    u, sc, dx, W1, b1, W2, b2 = problem(case, dtype)
    fw = forward(ops, case, dtype, u, sc, W1, b1, W2, b2)
    z, hh, s, x = R.se_forward64(u, sc, W1, b1, W2, b2)
    assert (hh[:, ::3] == 0).all() and (hh > 0).any()                       # the inactive units are inactive, others are not
    if h * w >= 64:
        assert s.min() < 0.2 and s.max() > 0.8                              # the gates are spread
    # squeeze: the chunk partials add up to the per-image channel sums
    part = host(fw["ws"]).astype(np.float64).reshape(n, fw["chunks"], c)
    close(part.sum(1), u.astype(np.float64).sum(axis=(1, 2)), tol(u.astype(np.float64).sum(axis=(1, 2)), "fp32"), "squeeze sums")
    close(fw["z"], z, tol(z, "fp32"), "z")
    close(fw["h"], hh, tol(hh, "fp32"), "h")
    assert (host(fw["h"])[:, ::3] == 0).all()
    close(fw["s"], s, tol(s, "fp32"), "s")
    close(fw["x"], x, tol(x, dtype), "x")
    # the statistics table: summed over its columns in float64 = per-channel sum / sum of squares of the STORED x
    xs = host(fw["x"]).astype(np.float64).reshape(-1, c)
    tab = host(fw["table"]).astype(np.float64)
    assert not np.isnan(tab).any()
    np.testing.assert_allclose(tab[0].sum(1), xs.sum(0), rtol=1e-4, atol=1e-2)
    np.testing.assert_allclose(tab[1].sum(1), (xs * xs).sum(0), rtol=1e-4, atol=1e-2)
    # ... and stp_bn_finalize takes it as it is
    from segmentation_training_pipeline_amd import _lib
    mean, rstd = nans((c,), "fp32"), nans((c,), "fp32")
    _lib.call("stp_bn_finalize", fw["table"].data_ptr(), n * fw["chunks"], xs.shape[0], c, 2e-5, 0.99, mean.data_ptr(), rstd.data_ptr(), None, None,
              torch.cuda.current_stream().cuda_stream)
    np.testing.assert_allclose(host(mean), xs.mean(0), rtol=1e-5)
    np.testing.assert_allclose(host(rstd), 1.0 / np.sqrt(xs.var(0) + 2e-5), rtol=1e-5)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", CASES, ids=lambda c: "%dx%dx%dx%d" % c)
def test_se_inference_form_writes_the_same_tensor(ops, case, dtype):
    u, sc, dx, W1, b1, W2, b2 = problem(case, dtype)
    a = forward(ops, case, dtype, u, sc, W1, b1, W2, b2, stats=True)
    b = forward(ops, case, dtype, u, sc, W1, b1, W2, b2, stats=False)
    assert bits_equal(host(b["x"]), host(a["x"]))
    _, _, _, x = R.se_forward64(u, sc, W1, b1, W2, b2)
    close(b["x"], x, tol(x, dtype), "x (inference form)")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", CASES, ids=lambda c: "%dx%dx%dx%d" % c)
def test_se_backward_matches_float64(ops, case, dtype):
    n, h, w, c = case
    u, sc, dx, W1, b1, W2, b2 = problem(case, dtype)
    fw = forward(ops, case, dtype, u, sc, W1, b1, W2, b2)
    got = backward(ops, case, dtype, fw, dx)
    # the reference backward starts from the DEVICE's fp32 z, h, s (their own parity is the forward test's): the gradients are then
    # compared at the same point, to the fp32 bound
    z, hh, s = (host(fw[k]).astype(np.float64) for k in ("z", "h", "s"))
    ref = R.se_backward64(dx, u, W1, W2, z, hh, s)
    part = host(got["ws"]).astype(np.float64).reshape(n, fw["chunks"], c)
    close(part.sum(1), ref["ds"], tol(ref["ds"], "fp32"), "ds")
    for k in ("da2", "da1", "dz", "dW1", "db1", "dW2", "db2"):
        close(got[k], ref[k], tol(ref[k], "fp32"), k)
    assert (host(got["da1"])[:, ::3] == 0).all()                           # the ReLU mask
    close(got["du"], ref["du"], tol(ref["du"], dtype), "du")


@pytest.mark.parametrize("dtype", DTYPES)
def test_se_backward_matches_float64_autograd(ops, dtype):
    """The formulas themselves: the float64 restatement the other tests compare with equals torch float64 autograd."""
    case = (3, 24, 40, 128)
    u, sc, dx, W1, b1, W2, b2 = problem(case, dtype)
    t = {k: torch.tensor(v.astype(np.float64), requires_grad=True) for k, v in dict(u=u, sc=sc, W1=W1, b1=b1, W2=W2, b2=b2).items()}
    z = t["u"].mean(dim=(1, 2))
    hh = torch.relu(z @ t["W1"] + t["b1"])
    s = torch.sigmoid(hh @ t["W2"] + t["b2"])
    x = t["u"] * s[:, None, None, :] + t["sc"]
    x.backward(torch.tensor(dx.astype(np.float64)))
    ref = R.se_backward64(dx, u, W1, W2, z.detach().numpy(), hh.detach().numpy(), s.detach().numpy())
    for k, name in (("u", "du"), ("W1", "dW1"), ("b1", "db1"), ("W2", "dW2"), ("b2", "db2")):
        np.testing.assert_allclose(ref[name], t[k].grad.numpy(), rtol=1e-10, atol=1e-13)
    np.testing.assert_allclose(t["sc"].grad.numpy(), dx.astype(np.float64))
    # ... and the device agrees with autograd end to end (forward error included) at the stored tensor's bound
    fw = forward(ops, case, dtype, u, sc, W1, b1, W2, b2)
    got = backward(ops, case, dtype, fw, dx)
    close(got["du"], t["u"].grad.numpy(), tol(t["u"].grad.numpy(), dtype), "du vs autograd")
    for k, name in (("W1", "dW1"), ("b1", "db1"), ("W2", "dW2"), ("b2", "db2")):
        close(got[name], t[k].grad.numpy(), tol(t[k].grad.numpy(), "fp32"), name + " vs autograd")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", [(3, 24, 40, 128), (4, 64, 64, 256), (1100, 2, 2, 64)], ids=lambda c: "%dx%dx%dx%d" % c)
def test_se_two_calls_are_bit_identical(ops, case, dtype):
    u, sc, dx, W1, b1, W2, b2 = problem(case, dtype)
    runs = []
    for _ in range(2):
        fw = forward(ops, case, dtype, u, sc, W1, b1, W2, b2)
        bw = backward(ops, case, dtype, fw, dx)
        runs.append({k: host(v) for k, v in list(fw.items()) + list(bw.items()) if isinstance(v, torch.Tensor) and k not in ("u", "W1", "W2")})
    assert sorted(runs[0]) == sorted(["ws", "z", "h", "s", "x", "table", "da2", "da1", "dz", "dW1", "db1", "dW2", "db2", "du"])
    for k in runs[0]:
        assert bits_equal(runs[1][k], runs[0][k]), k


def test_se_parameter_gradients_are_written_not_accumulated(ops):
    case, dtype = (2, 16, 16, 64), "bf16"
    u, sc, dx, W1, b1, W2, b2 = problem(case, dtype)
    fw = forward(ops, case, dtype, u, sc, W1, b1, W2, b2)
    a = backward(ops, case, dtype, fw, dx)
    n, h, w, c = case
    r = c // 16
    first = {k: host(a[k]).copy() for k in ("dW1", "db1", "dW2", "db2")}
    # the same buffers again (the gradient arena is zeroed once, when the plan is built: every step overwrites)
    ops.se_excite_bwd(a["ws"], n, h * w, c, r, fw["W1"], fw["W2"], fw["z"], fw["h"], fw["s"], a["da2"], a["da1"], a["dz"], a["dW1"], a["db1"],
                      a["dW2"], a["db2"])
    for k, v in first.items():
        assert bits_equal(host(a[k]), v), k


@pytest.mark.parametrize("dtype", DTYPES)
def test_se_refusals(ops, dtype):
    from segmentation_training_pipeline_amd import _lib
    st = torch.cuda.current_stream().cuda_stream
    other = {"fp32": None, "bf16": _lib.F16, "fp16": _lib.BF16}[dtype]
    cdt = {"fp32": _lib.F32, "bf16": _lib.BF16, "fp16": _lib.F16}[dtype]
    n, hw, c, r = 2, 64, 64, 4
    t = dev(np.zeros((n, hw, c)), dtype)
    y = nans((n, hw, c), dtype)
    v = f32(np.zeros(4096))
    p = lambda a: a.data_ptr()      # noqa: E731
    # channel counts the kernels do not serve: C % 8 != 0, C / 16 < 1, C > 512; hidden units out of range
    for bad_c in (12, 68, 8, 520, 1024):
        assert rc("stp_se_chunks", n, hw, bad_c) == 0 and rc("stp_se_workspace_bytes", n, hw, bad_c) == 0
        assert rc("stp_se_squeeze", p(t), cdt, n, hw, bad_c, p(v), 4 * v.numel(), st) == BADARG
        assert rc("stp_se_excite", p(v), n, hw, bad_c, r, p(v), p(v), p(v), p(v), p(v), p(v), p(v), st) == BADARG
        assert rc("stp_se_scale_add", p(t), p(t), p(y), cdt, n, hw, bad_c, p(v), None, st) == BADARG
        assert rc("stp_se_bwd_reduce", p(t), p(t), cdt, n, hw, bad_c, p(v), 4 * v.numel(), st) == BADARG
        assert rc("stp_se_excite_bwd", p(v), n, hw, bad_c, r, *([p(v)] * 12), st) == BADARG
        assert rc("stp_se_bwd_apply", p(t), p(y), cdt, n, hw, bad_c, p(v), p(v), st) == BADARG
    for bad_r in (0, 33, 128):
        assert rc("stp_se_excite", p(v), n, hw, c, bad_r, p(v), p(v), p(v), p(v), p(v), p(v), p(v), st) == BADARG
        assert rc("stp_se_excite_bwd", p(v), n, hw, c, bad_r, *([p(v)] * 12), st) == BADARG
    # a workspace that is too small, missing operands, the other build's 16-bit format, empty extents
    assert rc("stp_se_squeeze", p(t), cdt, n, hw, c, p(v), 4 * n * c - 4, st) == -3
    assert rc("stp_se_bwd_reduce", p(t), p(t), cdt, n, hw, c, p(v), 0, st) == -3
    assert rc("stp_se_squeeze", None, cdt, n, hw, c, p(v), 4 * v.numel(), st) == BADARG
    assert rc("stp_se_scale_add", p(t), None, p(y), cdt, n, hw, c, p(v), None, st) == BADARG
    assert rc("stp_se_bwd_apply", p(t), p(y), cdt, n, hw, c, None, p(v), st) == BADARG
    if other is not None:
        assert rc("stp_se_squeeze", p(t), other, n, hw, c, p(v), 4 * v.numel(), st) == BADARG
        assert rc("stp_se_scale_add", p(t), p(t), p(y), other, n, hw, c, p(v), None, st) == BADARG
        assert rc("stp_se_bwd_apply", p(t), p(y), other, n, hw, c, p(v), p(v), st) == BADARG
    assert rc("stp_se_squeeze", p(t), cdt, 0, hw, c, p(v), 4 * v.numel(), st) == BADARG
    assert rc("stp_se_scale_add", p(t), p(t), p(y), cdt, n, 0, c, p(v), None, st) == BADARG
    torch.cuda.synchronize()
    assert np.isnan(host(y)).all()              # a refused call launches nothing
