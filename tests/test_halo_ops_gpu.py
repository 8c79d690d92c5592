"""GPU op tests of the halo-resident convolution kernel (csrc/conv_halo.hip): everything stp_conv2d reaches with tile = 1024 + variant -
forward, the stride-1 data gradient, the space-to-depth stride-2 data gradient; six tile variants, the two-source / nearest-2x form,
the fused producer BatchNormalization, the folded 1x1 sibling, the persistent 64 -> 64 form, the four row-major epilogues and the group
pre-reduction - in both 16-bit builds (the kernel has no fp32 build: asserted).  Every launch goes through stp_conv2d with a forced
tile and is compared with the float64 numpy restatement of tests/_halo_reference.py - never with a second kernel, with no tolerance
scaled by a tensor's largest element and none taken from a kernel's output.  Two comparisons only:

* EXACT: integer operands, bias, residual and priors; BatchNormalization constants integer with rstd 1, as the identity and as one
  affine instance (mean 1, gamma 2, beta 3: the padding of the NORMALISED tensor is then visible); mask inputs include -0.0, 0, the
  smallest positive storage value, 6 and 7.  tests/test_halo_reference_host.py asserts on these very inputs that every sum of absolute
  terms - per element, per statistic column, per bnb column - stays below 2^24, so any order of fp32 additions is exact: the stored
  tensor equals q(reference) bit for bit and every statistic column equals the exact sums of one tile.  include/stp_hip.h says
  [2][C][pixel tiles] and does not say which tile is which column, so the table is compared as the MULTISET of its per-tile column
  vectors (columns sorted lexicographically), never as a total; stats_group_out, whose header text fixes "tile order", column by column.
* ROUNDED: normal operands rounded to storage first; storage rounding is monotonic, so q(ref - e) <= got <= q(ref + e) element by
  element with e = (n + 2) 2^-24 abs_terms of the element's own terms.  Only elements whose re-derived pre-activation lies within its
  own fma rounding of a clamp edge are left out (at most 0.5 %, asserted).  The tables are bounded the same way from the STORED tensor,
  column by column in the order image, tile row, tile column that conv_halo.hip gives them (a bound needs an assignment; the exact
  class has shown the multiset).  With a fused producer BatchNormalization the reference is taken over the tensor stp_bn_apply wrote.

Every destination is pre-filled with NaN (or the known prior where the launch accumulates) and carries 64 canary elements behind it;
stats_partial, stats_group_out and the counters are EXACTLY the queried size, NaN-filled (counters zero), with a canary behind them;
canaries are compared bit for bit after every launch; every launch runs twice and the bytes of the outputs and tables are compared;
refusals are checked on the return code, last, with nothing read afterwards.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _halo_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
TD = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
CANARY = 64
CANARY_BITS = {2: 0x5CA1, 4: 0x5CA1AB1E}
CLASSES = ["exact", "rounded"]


def q(a, dtype):
    """tests/test_ops_gpu.py's helper: a numpy array rounded through the storage dtype."""
    from test_ops_gpu import q as q_
    return q_(a, dtype)


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from segmentation_training_pipeline_amd import ops as o
    return o


@pytest.fixture(autouse=True)
def _storage_build(request):
    """Tests parametrized with dtype "fp16" call into libstp_hip_f16.so (IEEE-half storage)."""
    from segmentation_training_pipeline_amd import _lib
    dt = request.node.callspec.params.get("dtype") if hasattr(request.node, "callspec") else None
    with _lib.storage("fp16" if dt == "fp16" else "bf16"):
        yield


_KEEP = []


def keep(t):
    _KEEP.append(t)
    return t


@pytest.fixture(autouse=True)
def _release_device_temporaries():
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:      # a device fault ends the run: nothing more is started on that GPU
        pytest.exit("the GPU reported %s" % e, returncode=3)
    del _KEEP[:]


def dev(a, dtype):
    """Device copy in the storage dtype, parked until the test ends (the C-ABI holds raw pointers only)."""
    return keep(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(TD[dtype]).to(DEV).contiguous())


def f32(a):
    return keep(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV))


def host(t):
    torch.cuda.synchronize()
    return t.detach().to(torch.float32).cpu().numpy()


def lib():
    from segmentation_training_pipeline_amd import _lib
    return _lib.load()


def stream():
    return torch.cuda.current_stream().cuda_stream


class Guarded(object):
    """``shape`` elements of device memory of a torch dtype with CANARY canary elements directly behind them."""

    def __init__(self, shape, tdtype):
        self.shape = tuple(int(s) for s in np.atleast_1d(shape))
        self.n = int(np.prod(self.shape))
        self.buf = keep(torch.empty(self.n + CANARY, dtype=tdtype, device=DEV))
        self.data = self.buf[:self.n]
        size = self.buf.element_size()
        self.bits = CANARY_BITS[size]
        self.canary = self.buf[self.n:].view(torch.int16 if size == 2 else torch.int32)
        self.canary.fill_(self.bits)
        self.integer = not tdtype.is_floating_point

    def ptr(self):
        return self.buf.data_ptr()

    def fill(self, values=None):
        """NaN (zero for the counters), or the given prior contents."""
        if values is None:
            self.data.fill_(0 if self.integer else float("nan"))
        else:
            self.data.copy_(torch.from_numpy(np.ascontiguousarray(values, dtype=np.float32).reshape(-1)).to(self.data.dtype))

    def intact(self):
        torch.cuda.synchronize()
        return bool((self.canary == self.bits).all().item())

    def read(self):
        torch.cuda.synchronize()
        if self.integer:
            return self.data.cpu().numpy().copy().reshape(self.shape)
        return host(self.data).copy().reshape(self.shape)


class Launch(object):
    """One stp_conv2d launch of (case, mode) on the device: operands, guarded destinations and tables of exactly the queried size."""

    def __init__(self, case, mode, klass, dtype, group=0):
        from segmentation_training_pipeline_amd import _lib
        self.case, self.mode, self.klass, self.dtype = case, mode, klass, dtype
        d, o = R.inputs(case, klass, dtype), R.options(case, mode)
        self.d, self.o = d, o
        co = R.cout_of(case, mode)
        cd0 = min(o.cd0, co)
        w = R.device_weights(case, klass, dtype)
        src0 = R.pbn_source(case, klass, dtype, o.params) if o.pbn is not None else d["x0"]
        self.src0_pre = dev(src0, dtype)
        ptr = dict(src0=self.src0_pre.data_ptr(), weight=dev(w["weight"], dtype).data_ptr())
        if case.c1:
            ptr["src1"] = dev(d["x1"], dtype).data_ptr()
        if w["fold_weight"] is not None:
            ptr["fold_weight"] = dev(w["fold_weight"], dtype).data_ptr()
        if case.fold_c:
            ptr["fold_src"] = dev(d["fold_src"], dtype).data_ptr()
        if o.bias:
            ptr["bias"] = f32(d["bias"][:co]).data_ptr()
        if o.residual:
            ptr["residual"] = dev(d["residual"][..., :co], dtype).data_ptr()
        self.bn = None
        if o.bnb is not None:
            self.bn = R.bnb_params_of(case, klass, dtype, o.params)
            ptr["bnb_x"] = dev(d["bnb_x"], dtype).data_ptr()
            for name, a in zip(("bnb_mean", "bnb_rstd", "bnb_gamma", "bnb_beta"), self.bn):
                ptr[name] = f32(a).data_ptr()
        if o.pbn is not None:
            self.bn = R.pbn_params_of(case, klass, dtype, o.params)
            for name, a in zip(("pbn_mean", "pbn_rstd", "pbn_gamma", "pbn_beta"), self.bn):
                ptr[name] = f32(a).data_ptr()
        if o.sum2x2:
            shape0, self.prior0 = (case.n, case.h // 2, case.w // 2, cd0), (d["prior_low"] if o.acc0 else None)
        elif case.s2d:
            shape0, self.prior0 = (case.n, 2 * case.h, 2 * case.w, case.co // 4), (d["prior0"] if o.acc0 else None)
        else:
            shape0, self.prior0 = (case.n, case.h, case.w, cd0), (d["prior"][..., :cd0] if o.acc0 else None)
        self.dst0 = Guarded(shape0, TD[dtype])
        ptr["dst0"] = self.dst0.ptr()
        self.dst1 = self.prior1 = None
        if cd0 < co:
            self.dst1 = Guarded((case.n, case.h, case.w, co - cd0), TD[dtype])
            self.prior1 = d["prior"][..., cd0:co] if o.acc1 else None
            ptr["dst1"] = self.dst1.ptr()
        self.stats = None
        if o.stats:
            self.stats = Guarded((R.stats_floats(case, mode),), torch.float32)
            ptr["stats"] = self.stats.ptr()
        self.P = R.fill_params(_lib.ConvParams(), case, mode, dtype, ptr)
        if o.stats:
            assert int(lib().stp_conv2d_stats_floats(C.byref(self.P))) == self.stats.n, "stp_conv2d_stats_floats"
        self.group_out = self.counters = None
        if group:
            cs = R.stat_channels(case, mode)
            self.group_out = Guarded((2 * cs * -(-R.tiles_of(case) // group),), torch.float32)
            self.counters = Guarded((int(lib().stp_conv2d_stats_group_counters(C.byref(self.P), group)),), torch.int32)
            self.counters.fill()
            self.P.stats_group_out, self.P.stats_group_counters, self.P.stats_group = self.group_out.ptr(), self.counters.ptr(), group

    def buffers(self):
        return [b for b in (self.dst0, self.dst1, self.stats, self.group_out, self.counters) if b is not None]

    def run(self):
        """-> dict of what the launch left (canaries and counters checked)."""
        self.dst0.fill(self.prior0)
        if self.dst1 is not None:
            self.dst1.fill(self.prior1)
        for b in (self.stats, self.group_out):
            if b is not None:
                b.fill()
        rc = int(lib().stp_conv2d(C.byref(self.P), stream()))
        assert rc == 0, "stp_conv2d(%s %s %s): %d" % (self.case.family, self.case.name, self.mode, rc)
        out = dict(dst0=self.dst0.read(), dst1=None if self.dst1 is None else self.dst1.read(), stats=None if self.stats is None else self.stats.read(),
                   group=None if self.group_out is None else self.group_out.read())
        for b in self.buffers():
            assert b.intact(), "%s %s %s wrote behind a buffer of %d elements" % (self.case.family, self.case.name, self.mode, b.n)
        if self.counters is not None:
            assert not self.counters.read().any(), "the group counters are not back at zero"
        if self.stats is not None:
            assert int(self.P.stats_tiles) * 2 * R.stat_channels(self.case, self.mode) == self.stats.n
        return out

    def twice(self):
        a, b = self.run(), self.run()
        for k in a:
            assert (a[k] is None) == (b[k] is None) and (a[k] is None or a[k].tobytes() == b[k].tobytes()), "%s: a second identical launch gave different bytes" % k
        return a

    def refused(self):
        """Return code of a launch that must not start (nothing is synchronised or read afterwards)."""
        return int(lib().stp_conv2d(C.byref(self.P), stream()))


def check_stored(klass, got, dst, dtype, what):
    """EXACT: equal to q(reference) as numbers, nothing left unwritten.  ROUNDED: inside [q(ref - e), q(ref + e)] element by element."""
    assert not np.isnan(got).any(), "%s: %d elements were not written" % (what, int(np.isnan(got).sum()))
    ref = q(R.stored_reference(dst), dtype)
    assert got.shape == ref.shape
    if klass == "exact":
        bad = got != ref
        assert not bad.any(), "%s: %d of %d elements differ from the rounded exact sum, first at %s: %r against %r" % (
            what, int(bad.sum()), bad.size, tuple(np.argwhere(bad)[0]), float(got[bad][0]), float(ref[bad][0]))
        return ref
    lo, hi = R.stored_bounds(dst)
    lo, hi = q(lo, dtype), q(hi, dtype)
    near = dst["near"] if dst["near"] is not None else np.zeros(got.shape, bool)
    assert float(near.mean()) <= R.MASK_SHARE_CAP, "%s: %.4f of the elements sit on a clamp edge" % (what, float(near.mean()))
    bad = ((got < lo) | (got > hi)) & ~near
    # what can be observed behind a storage rounding: where the stored value is not q(ref), the fp32 sum lay beyond the rounding boundary
    # between the two, so its error was at least the reference's distance to that boundary - as a share of the element's own bound e
    moved = (got != ref) & ~near
    e = np.maximum(R.rounding_bound(dst["n"], dst["abs"]), 1e-300)
    needed = np.abs((got.astype(np.float64) + ref) / 2 - R.stored_reference(dst)) / e
    print("HALO_STORED %s: %.5f of the elements differ from q(ref), least error / e that explains them = %.4f; %d left out at a clamp edge" % (
        what, float(moved.mean()), float(needed[moved].max()) if moved.any() else 0.0, int(near.sum())))
    assert not bad.any(), "%s: %d of %d elements outside [q(ref - e), q(ref + e)], first at %s: %r against [%r, %r]" % (
        what, int(bad.sum()), bad.size, tuple(np.argwhere(bad)[0]), float(got[bad][0]), float(lo[bad][0]), float(hi[bad][0]))
    if near.any():      # an element on the edge holds the masked or the unmasked value, nothing else
        v = R.rounding_bound(dst["n"], dst["abs"])
        free = near & ~((got == 0) | ((got >= q(dst["pre"] - v, dtype)) & (got <= q(dst["pre"] + v, dtype))))
        assert not free.any(), "%s: an element at a clamp edge holds neither 0 nor the gradient" % what
    return got


def check_tables(klass, got, case, mode, stored, bnb, what):
    """``stored``: EXACT - q(reference) (the launch's tensor equals it, asserted before); ROUNDED - what the launch stored."""
    t = R.tables(case, mode, stored, bnb)
    rows = t["value"].shape[0] * t["value"].shape[1]
    got2, ref2, slack2 = got.reshape(rows, -1).astype(np.float64), t["value"].reshape(rows, -1), t["slack"].reshape(rows, -1)
    assert got2.shape == ref2.shape and not np.isnan(got2).any(), "%s: %d table entries were not written" % (what, int(np.isnan(got2).sum()))
    if klass == "exact":
        loose = slack2.any(axis=1)      # at most the one row whose input holds the smallest positive storage value (g * tiny is no integer)
        assert int(loose.sum()) <= 1
        a, b = R.sort_columns(got2[~loose]), R.sort_columns(ref2[~loose])
        bad = (a != b).any(axis=0)
        assert not bad.any(), "%s: %d of %d statistic columns are not the exact sums of one tile" % (what, int(bad.sum()), bad.size)
        for r in np.flatnonzero(loose):
            assert (np.abs(np.sort(got2[r]) - np.sort(ref2[r])) <= slack2[r].max()).all(), "%s: row %d" % (what, r)
        return
    bound = R.rounding_bound(t["n"], t["abs"]).reshape(rows, -1) + slack2
    err = np.abs(got2 - ref2)
    print("HALO_TABLE %s: max error / bound = %.4f" % (what, float((err / np.maximum(bound, 1e-300)).max())))
    bad = err > bound
    assert not bad.any(), "%s: %d of %d table entries outside the bound, worst %.3g against %.3g" % (
        what, int(bad.sum()), bad.size, float(err[bad].max()), float(bound[bad][err[bad].argmax()]))


def run_and_check(case, mode, klass, dtype, act=None, launch=None):
    """One (case, mode): the launch twice, the stored tensors, the tables.  -> (launch, outputs, reference)."""
    L = launch or Launch(case, mode, klass, dtype)
    what = "%s/%s/%s/%s/%s" % (case.family, case.name, mode, dtype, klass)
    assert int(lib().stp_conv2d_tile_for(C.byref(L.P))) == 1024 + case.v, what
    out = L.twice()
    r = R.launch_reference(case, mode, klass, dtype, act=act)
    stored = [check_stored(klass, out["dst0"], r["dst0"], dtype, what + " dst0")]
    if r["dst1"] is not None:
        stored.append(check_stored(klass, out["dst1"], r["dst1"], dtype, what + " dst1"))
    else:
        assert out["dst1"] is None
    if out["stats"] is not None:
        check_tables(klass, out["stats"], case, mode, stored[0] if L.o.sum2x2 else np.concatenate(stored, axis=-1), r["bnb"], what)
    return L, out, r


def ids(v):
    return v if isinstance(v, str) else "%s-%s" % (v.family, v.name)


def params_of(cases):
    return [(c, dt, k) for c in cases for dt in R.H16 for k in CLASSES if not (c.exact_only and k != "exact")]


# ---------------------------------------------------------------------------------------------------------------------------------
# one source (conv_halo_kernel / conv_halo_p64_kernel): plain (EP 0), fused statistics (EP 1), the epilogue operands

@pytest.mark.parametrize("case,dtype,klass", params_of(R.ONE_CASES), ids=ids)
def test_one_source(ops, case, dtype, klass):
    for mode in R.modes_of(case, klass):
        if mode == "two_dst" and case.v == 5:
            continue                                       # (refused: below, last)
        run_and_check(case, mode, klass, dtype)
    if case.v == 5 and "two_dst" in R.modes_of(case, klass):      # the persistent 64 -> 64 form has ONE destination
        assert Launch(case, "two_dst", klass, dtype).refused() == R.BADARG


@pytest.mark.parametrize("dtype", R.H16)
def test_persistent_form_second_trip_of_the_tile_loop(ops, dtype):
    """3 x 88 x 256 pixels = 528 tiles of 8 x 16 against 2 x compute units persistent workgroups: 16 of them take a second tile, the
    others do not (the ragged second trip).  Exact class only; plain and with the fused statistics."""
    case = R.ONE_MULTI_TRIP
    assert R.tiles_of(case) > 2 * torch.cuda.get_device_properties(0).multi_processor_count
    for mode in R.ONE_MODES:
        run_and_check(case, mode, "exact", dtype)


# ---------------------------------------------------------------------------------------------------------------------------------
# two sources, the first optionally behind UpSampling2D(2) (conv_halo2_kernel)

@pytest.mark.parametrize("case,dtype,klass", params_of(R.TWO_CASES), ids=ids)
def test_two_sources(ops, case, dtype, klass):
    for mode in R.modes_of(case, klass):
        run_and_check(case, mode, klass, dtype)


# ---------------------------------------------------------------------------------------------------------------------------------
# fused producer BatchNormalization (conv_halo_pbn_kernel), each with the fused statistics of the output

@pytest.mark.parametrize("case,dtype,klass", params_of(R.PBN_CASES), ids=ids)
def test_fused_producer_batchnorm(ops, case, dtype, klass):
    for mode in R.modes_of(case, klass):
        L = Launch(case, mode, klass, dtype)
        act = None
        if klass == "rounded":      # the reference runs over the normalised tensor as stp_bn_apply writes it
            t = keep(torch.empty_like(L.src0_pre))
            mean, rstd, gamma, beta = [f32(a) for a in L.bn]
            ops.bn_apply(L.src0_pre, t, case.n * case.h * case.w, case.c0, case.c0, mean, rstd, gamma, beta, relu=L.o.pbn)
            act = host(t)
        run_and_check(case, mode, klass, dtype, act=act, launch=L)


# ---------------------------------------------------------------------------------------------------------------------------------
# BatchNormalization-backward epilogue (EP 2): bnb_relu 0 / 1 / 2, as first and as last consumer

@pytest.mark.parametrize("case,dtype,klass", params_of(R.BNB_CASES), ids=ids)
def test_batchnorm_backward_epilogue(ops, case, dtype, klass):
    for mode in R.modes_of(case, klass):
        run_and_check(case, mode, klass, dtype)


# ---------------------------------------------------------------------------------------------------------------------------------
# 2 x 2-summed destination (EP 3), with a second destination and as the one-destination form

@pytest.mark.parametrize("case,dtype,klass", params_of([c for c in R.SUM_CASES if c is not R.SUM_REFUSED]), ids=ids)
def test_summed_destination(ops, case, dtype, klass):
    for mode in R.modes_of(case, klass):
        run_and_check(case, mode, klass, dtype)


# ---------------------------------------------------------------------------------------------------------------------------------
# space-to-depth stride-2 data gradient (conv_halo_s2d_kernel) and the stride-1 fold (conv_halo_fold1_kernel)

@pytest.mark.parametrize("case,dtype,klass", params_of(R.S2D_CASES), ids=ids)
def test_space_to_depth_data_gradient(ops, case, dtype, klass):
    for mode in R.modes_of(case, klass):
        run_and_check(case, mode, klass, dtype)


@pytest.mark.parametrize("case,dtype,klass", params_of(R.FOLD_CASES), ids=ids)
def test_stride1_fold(ops, case, dtype, klass):
    for mode in R.modes_of(case, klass):
        run_and_check(case, mode, klass, dtype)


# ---------------------------------------------------------------------------------------------------------------------------------
# group pre-reduction: the switch is read once per process

def group_pre_reduction(dtype):
    """147 tiles, G = 2, 74 groups with the last one short: stats_partial as the multiset of exact tile columns, stats_group_out column by
    column - the header fixes it: the group's columns summed in tile order - counters back at zero, a replay bit-identical."""
    case = R.GROUP_CASE
    probe = Launch(case, "stats", "exact", dtype)
    G = int(lib().stp_conv2d_stats_group_for(C.byref(probe.P)))
    assert G == 2, "stp_conv2d_stats_group_for = %d (STP_STATS_GROUP=1 is needed)" % G
    L = Launch(case, "stats", "exact", dtype, group=G)
    assert L.counters.n == 4 * 74
    _, out, r = run_and_check(case, "stats", "exact", dtype, launch=L)
    t = R.tables(case, "stats", q(R.stored_reference(r["dst0"]), dtype))
    want = R.group_table(t["value"], G)
    got = out["group"].reshape(want.shape)
    assert not np.isnan(got).any() and np.array_equal(got, want), "stats_group_out differs from the tile-order sums of its groups"
    L.P.stats_group = 4                                    # a group size the kernel would not choose is refused
    assert L.refused() == R.BADARG


def test_group_pre_reduction_in_its_own_process():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, STP_STATS_GROUP="1", PYTHONPATH=os.pathsep.join([root, os.path.join(root, "tests")]))
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=300, cwd=root)
    assert r.returncode == 0 and "GROUP_OK bf16 fp16" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


# ---------------------------------------------------------------------------------------------------------------------------------
# what the library refuses

@pytest.mark.parametrize("dtype", R.H16)
def test_no_fp32_build(ops, dtype):
    from segmentation_training_pipeline_amd import _lib
    fake = dict.fromkeys("src0 src1 weight bias residual dst0 dst1 stats".split(), 0x10000)
    for case in R.ONE_CASES + R.TWO_CASES:
        P = R.fill_params(_lib.ConvParams(), case, "plain", "fp32", fake)
        assert int(lib().stp_conv2d_tile_for(C.byref(P))) == R.BADARG and int(lib().stp_conv2d_halo_variant(C.byref(P))) == -1


@pytest.mark.parametrize("dtype", R.H16)
def test_refusals(ops, dtype):
    """STP_E_BADARG, nothing launched: every pointer names one zeroed scratch buffer larger than any operand of these shapes."""
    from segmentation_training_pipeline_amd import _lib
    scratch = keep(torch.zeros(8 << 20, dtype=torch.uint8, device=DEV))
    names = "src0 src1 weight bias residual dst0 dst1 stats bnb_x bnb_mean bnb_rstd bnb_gamma bnb_beta pbn_mean pbn_rstd pbn_gamma pbn_beta fold_src fold_weight"
    ptr = dict.fromkeys(names.split(), scratch.data_ptr())
    torch.cuda.synchronize()
    rcs = []
    for case, mode, what in R.REFUSALS:
        P = R.fill_params(_lib.ConvParams(), case, mode, dtype, ptr)
        planned = int(lib().stp_conv2d_halo_variant(C.byref(P)))
        assert planned == (case.v if what in R.LAUNCH_LEVEL_REFUSALS else -1), what
        rcs.append((what, int(lib().stp_conv2d(C.byref(P), stream()))))
    assert all(rc == R.BADARG for _, rc in rcs), rcs


if __name__ == "__main__":
    from segmentation_training_pipeline_amd import _lib as _l
    done = []
    for _dtype in R.H16:
        with _l.storage(_dtype):
            group_pre_reduction(_dtype)
        torch.cuda.synchronize()
        del _KEEP[:]
        done.append(_dtype)
    print("GROUP_OK " + " ".join(done))
