"""GPU op tests of the small-channel forward / data-gradient kernels and the stem: everything stp_conv2d reaches with tile id 512
(csrc/conv_sc.hip with conv_sc_epilogue.h - single-shot and streaming - and the lean kernels of conv_sc_lean.hip), 640 (conv_sc_wide.hip),
704 (conv_sc_narrow.hip) and 768 (conv_sc_stem.hip and the persistent stem kernel), in the fp32, bf16 and IEEE-half builds.  Every
launch goes through stp_conv2d with tile = 0 (the id and the kernel's eligibility query are asserted first) and is compared with the
float64 numpy restatement of tests/_sc_reference.py - never with a second kernel, with no bound scaled by a tensor's largest element
and none taken from a kernel's output.  Two comparisons only, DESIGN.md 3.33's:

* EXACT: integer operands, bias and priors; BatchNormalization constants integer with rstd 1, as the identity and as one affine
  instance (mean 1, gamma 2, beta 3); mask inputs include -0.0, 0, the smallest positive storage value, 6 and 7.
  tests/test_sc_reference_host.py asserts on these very inputs that every sum of absolute terms - per element, and per channel over
  the WHOLE tensor - stays below 2^24, so any order of fp32 additions and any tile-to-workgroup map is exact: the stored tensor equals
  q(reference) bit for bit; the columns of a table, summed in float64, equal the reference total; the slots add up to it in 2^-24 units.
* ROUNDED: normal operands rounded to storage first; q(ref - e) <= got <= q(ref + e) element by element with e = (n + 2) 2^-24 abs of
  the element's own terms (a 2 x 2-summed element: all four pixels' products plus the three additions).  Only elements whose re-derived
  pre-activation lies within its own fma rounding of a clamp edge are left out (at most 0.5 %, asserted; such an element must still
  hold 0 or the gradient).  Table totals are bounded the same way from the STORED tensor with the number of summed terms as n; the
  slots get 2^-25 of their abs more.  With a fused producer BatchNormalization the reference runs over the normalised tensor as
  stp_bn_apply wrote it (DESIGN.md 3.31 does the same).

The header does not say which tiles a persistent workgroup owns, so a table is checked as: exactly stp_conv2d_stats_floats(p) floats
and P.stats_tiles columns, every column written (they start as NaN), per-channel totals.  Destinations start as NaN (or the known
prior) with 64 canary elements behind them; tables, slots and the bnb / pbn constants are EXACTLY the queried size with a canary behind
them; canaries are compared bit for bit after every launch; every launch runs twice and the bytes of outputs and tables are
compared; refusals are checked on the return code, last, with nothing read afterwards.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _sc_reference as R
import test_igemm_ops_gpu as G
from test_igemm_ops_gpu import _release_device_temporaries, _storage_build, ops  # noqa: F401  (the fixtures: per-dtype library, device temporaries)

pytestmark = pytest.mark.gpu

Guarded, keep, dev, f32, q, lib, stream, TD, DEV = G.Guarded, G.keep, G.dev, G.f32, G.q, G.lib, G.stream, G.TD, G.DEV


def constants(values):
    """Per-channel fp32 constants of EXACTLY their size, with the canary behind them."""
    g = Guarded((len(values),), torch.float32)
    g.fill(values)
    return g


class Launch(object):
    """One stp_conv2d launch of (case, mode) on the device: operands, guarded destinations, constants and tables of exactly the queried size."""

    def __init__(self, case, mode, klass, dtype):
        from segmentation_training_pipeline_amd import _lib
        self.case, self.mode, self.klass, self.dtype = case, mode, klass, dtype
        d, o = R.inputs(case, klass, dtype), R.options(case, mode)
        self.d, self.o = d, o
        ho, wo = R.out_hw(case)
        cs = R.stat_channels(case)
        self.what = "%s/%s/%s/%s/%s" % (case.kind, case.name, mode, dtype, klass)
        self.src0 = dev(R.pbn_source(case, klass, dtype, o.params) if o.pbn is not None else d["x0"], dtype)
        ptr = dict(src0=self.src0.data_ptr(), weight=dev(R.device_weight(case, klass, dtype), dtype).data_ptr(), stats=0x10000)
        if case.kind == "scn":
            ptr["src1"] = dev(d["x1"], dtype).data_ptr()
        if o.bias:
            ptr["bias"] = f32(d["bias"]).data_ptr()
        self.guards = []
        self.bn = self.pbn = None
        if o.bnb is not None:
            self.bn = R.bnb_params_of(case, mode, klass, dtype)
            ptr["bnb_x"] = dev(d[R.bnb_key(case, mode)], dtype).data_ptr()
            for name, a in zip(("bnb_mean", "bnb_rstd", "bnb_gamma", "bnb_beta"), self.bn):
                self.guards.append(constants(a))
                ptr[name] = self.guards[-1].ptr()
        if o.pbn is not None:
            self.pbn = R.pbn_params_of(case, mode, klass, dtype)
            for name, a in zip(("pbn_mean", "pbn_rstd", "pbn_gamma", "pbn_beta"), self.pbn):
                self.guards.append(constants(a))
                ptr[name] = self.guards[-1].ptr()
        self.dst0 = Guarded(R.low_shape(case) if o.sum2 else (case.n, ho, wo, case.cout), TD[dtype])
        self.prior0 = (d["prior_low"] if o.sum2 else d["prior"]) if o.acc0 else None
        ptr["dst0"] = self.dst0.ptr()
        self.dst1 = self.prior1 = None
        if case.kind == "scw":
            self.dst1 = Guarded((case.n, ho, wo, case.cout - cs), TD[dtype])
            self.prior1 = d["prior"][..., cs:] if o.acc1 else None
            ptr["dst1"] = self.dst1.ptr()
        self.P = R.fill_params(_lib.ConvParams(), case, mode, dtype, ptr)
        self.stats = None
        if o.stats:
            self.floats = int(lib().stp_conv2d_stats_floats(C.byref(self.P)))
            assert self.floats > 0 and self.floats % (2 * cs) == 0, self.what
            self.stats = Guarded((2, cs, o.slots), torch.int64) if o.slots else Guarded((2, cs, self.floats // (2 * cs)), torch.float32)
            self.P.stats_partial = self.stats.ptr()

    def buffers(self):
        return [b for b in [self.dst0, self.dst1, self.stats] + self.guards if b is not None]

    def planned(self):
        """The plan facts, before anything is launched."""
        case = self.case
        assert int(self.P.tile) == 0 and int(lib().stp_conv2d_tile_for(C.byref(self.P))) == R.TILE[case.kind], self.what
        assert int(getattr(lib(), R.ELIGIBLE[case.kind])(C.byref(self.P))) == 1, self.what
        if case.exact_only:      # the trip loop: fewer columns (= persistent workgroups) than tiles, or the case does not test what it names
            cols = int(getattr(lib(), "stp_conv2d_%s_stats_tiles" % case.kind)(C.byref(self.P)))
            assert cols < R.tiles_of(case), "%s: %d workgroups for %d tiles - no second trip" % (self.what, cols, R.tiles_of(case))

    def run(self):
        """-> dict of what the launch left (canaries checked)."""
        self.dst0.fill(self.prior0)
        if self.dst1 is not None:
            self.dst1.fill(self.prior1)
        if self.stats is not None:
            self.stats.fill()
        rc = int(lib().stp_conv2d(C.byref(self.P), stream()))
        assert rc == 0, "stp_conv2d(%s): %d" % (self.what, rc)
        out = dict(dst0=self.dst0.read(), dst1=None if self.dst1 is None else self.dst1.read(), stats=None if self.stats is None else self.stats.read())
        for b in self.buffers():
            assert b.intact(), "%s wrote behind a buffer of %d elements" % (self.what, b.n)
        if self.stats is not None and not self.o.slots:
            assert int(self.P.stats_tiles) * 2 * R.stat_channels(self.case) == self.floats, "%s: P.stats_tiles = %d against %d floats" % (self.what, int(self.P.stats_tiles), self.floats)
            if self.case.exact_only:
                assert int(self.P.stats_tiles) < R.tiles_of(self.case), self.what
        return out

    def twice(self):
        a, b = self.run(), self.run()
        for k in a:
            assert (a[k] is None) == (b[k] is None) and (a[k] is None or a[k].tobytes() == b[k].tobytes()), "%s %s: a second identical launch gave different bytes" % (self.what, k)
        return a


def check_stored(klass, got, dst, dtype, what):
    """EXACT: equal to q(reference) as numbers, nothing left unwritten.  ROUNDED: inside [q(ref - e), q(ref + e)] element by element."""
    assert not np.isnan(got).any(), "%s: %d elements were not written" % (what, int(np.isnan(got).sum()))
    ref = q(R.stored_reference(dst), dtype)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
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
    e = np.maximum(R.rounding_bound(dst["n"], dst["abs"]), 1e-300)
    if dtype == "fp32":      # nothing hides behind a storage rounding: the error itself
        err = np.where(near, 0.0, np.abs(got.astype(np.float64) - R.stored_reference(dst))) / e
        print("SC_STORED %s: max error / e = %.4f; %d left out at a clamp edge" % (what, float(err.max()), int(near.sum())))
    else:
        # what can be observed behind a storage rounding: where the stored value is not q(ref), the fp32 sum lay beyond the rounding
        # boundary between the two, so its error was at least the reference's distance to that boundary - as a share of the bound e
        moved = (got != ref) & ~near
        needed = np.abs((got.astype(np.float64) + ref) / 2 - R.stored_reference(dst)) / e
        print("SC_STORED %s: %.5f of the elements differ from q(ref), least error / e that explains them = %.4f; %d left out at a clamp edge" % (
            what, float(moved.mean()), float(needed[moved].max()) if moved.any() else 0.0, int(near.sum())))
    assert not bad.any(), "%s: %d of %d elements outside [q(ref - e), q(ref + e)], first at %s: %r against [%r, %r]" % (
        what, int(bad.sum()), bad.size, tuple(np.argwhere(bad)[0]), float(got[bad][0]), float(lo[bad][0]), float(hi[bad][0]))
    if near.any():      # an element on the edge holds the masked or the unmasked value, nothing else
        v = R.rounding_bound(dst["n"], dst["abs"])
        free = near & ~((got == 0) | ((got >= q(dst["pre"] - v, dtype)) & (got <= q(dst["pre"] + v, dtype))))
        assert not free.any(), "%s: an element at a clamp edge holds neither 0 nor the gradient" % what
    return got


def check_table(klass, got, slots, stored, bnb, what):
    """``stored``: EXACT - q(reference) (the launch's tensor equals it, asserted before); ROUNDED - what the launch stored.  Every column
    written; per channel the float64 sum of the columns (the slots: in 2^-24 units) against the reference total."""
    t = R.totals(stored, bnb)
    if slots:
        assert got.dtype == np.int64 and got.shape == (2, stored.shape[-1], slots), (what, got.shape)
        total = got.sum(axis=-1).astype(np.float64) / R.SLOT_SCALE      # (integer sums below 2^53: exact)
    else:
        assert got.dtype == np.float32 and got.shape[:2] == (2, stored.shape[-1]), (what, got.shape)
        assert np.isfinite(got).all(), "%s: %d of %d table entries were not written" % (what, int((~np.isfinite(got)).sum()), got.size)
        total = got.astype(np.float64).sum(axis=-1)
    err = np.abs(total - t["value"])
    if klass == "exact":
        bad = err > t["slack"]
        assert not bad.any(), "%s: %d of %d channel totals differ from the exact sum, first %r against %r" % (
            what, int(bad.sum()), bad.size, float(total[bad][0]), float(t["value"][bad][0]))
        return
    bound = R.rounding_bound(t["n"], t["abs"]) + t["slack"] + (2.0 ** -25 * t["abs"] if slots else 0.0)
    print("SC_TABLE %s: max error / bound = %.4f" % (what, float((err / np.maximum(bound, 1e-300)).max())))
    bad = err > bound
    assert not bad.any(), "%s: %d of %d channel totals outside the bound, worst %.3g against %.3g" % (
        what, int(bad.sum()), bad.size, float(err[bad].max()), float(bound[bad][err[bad].argmax()]))


def run_and_check(case, mode, klass, dtype, ops=None):
    L = Launch(case, mode, klass, dtype)
    L.planned()
    act = None
    if L.o.pbn is not None and klass == "rounded":      # the reference runs over the normalised tensor as stp_bn_apply writes it
        t = keep(torch.empty_like(L.src0))
        c = R.cin_of(case, dtype)
        ops.bn_apply(L.src0, t, L.src0.numel() // c, c, c, *[f32(a) for a in L.pbn], relu=L.o.pbn)
        torch.cuda.synchronize()
        act = t.detach().to(torch.float32).cpu().numpy()
    out = L.twice()
    r = R.launch_reference(case, mode, klass, dtype, act=act)
    s0 = check_stored(klass, out["dst0"], r["dst0"], dtype, L.what + " dst0")
    if r["dst1"] is not None:
        check_stored(klass, out["dst1"], r["dst1"], dtype, L.what + " dst1")
    else:
        assert out["dst1"] is None
    if out["stats"] is not None:
        check_table(klass, out["stats"], L.o.slots, s0, r["bnb"], L.what)
    return L


def run_case(case, dtype, klass, ops):
    for mode in R.modes_of(case, klass):
        run_and_check(case, mode, klass, dtype, ops)


def ids(v):
    return v if isinstance(v, str) else "%s-%s" % (v.kind, v.name)


def params_of(cases):
    return [(c, dt, k) for c in cases for dt in R.DTYPES if dt in R.builds_of(c) for k in R.classes_of(c)]


# ---------------------------------------------------------------------------------------------------------------------------------
# id 512

@pytest.mark.parametrize("case,dtype,klass", params_of(R.SHAPE_CASES), ids=ids)
def test_shapes(ops, case, dtype, klass):
    """One partial tile, one full tile, a second tile row and column of one pixel, ragged in both directions - plain and with the fused
    statistics, every cin (partial last K chunk but for the widest) and every cout (lean, generic vector path, scalar tail, head)."""
    run_case(case, dtype, klass, ops)


@pytest.mark.parametrize("case,dtype,klass", params_of(R.MODE_CASES), ids=ids)
def test_every_mode_on_three_by_three_tiles(ops, case, dtype, klass):
    """1,21,67: the centre tile is interior (the lean kernel's unchecked path).  Epilogue operands (the scalar tail included), statistic
    columns and slots, the BatchNormalization-backward mask as first (lean) and as last consumer (generic), the fused producer
    BatchNormalization, the head with bias."""
    run_case(case, dtype, klass, ops)


@pytest.mark.parametrize("case,dtype,klass", params_of(R.SUM_CASES), ids=ids)
def test_summed_destination(ops, case, dtype, klass):
    """dst_sum2x2 on the even twins: plain, on top of a prior, with the mask and sums as first (lean: SCL_BNB_SUM2) and as last consumer
    (generic: accumulate0 together with bnb_x)."""
    run_case(case, dtype, klass, ops)


@pytest.mark.parametrize("case,dtype,klass", params_of(R.UP_CASES), ids=ids)
def test_upsampled_source(ops, case, dtype, klass):
    """NEAREST2X from 1,11,34: the lean UP form (statistics), with the producer BatchNormalization on the low-resolution pixels, and the
    generic kernel (accumulate)."""
    run_case(case, dtype, klass, ops)


# ---------------------------------------------------------------------------------------------------------------------------------
# ids 640, 704, 768

@pytest.mark.parametrize("case,dtype,klass", params_of(R.SCW_CASES), ids=ids)
def test_wide_output_two_destinations(ops, case, dtype, klass):
    """32 -> 128 with the first Cd0 channels summed at low resolution: Cd0 = 64 (the balanced wave split), 32 and 96 (wave * 32); each
    destination overwriting or accumulating; the mask and sums on dst0."""
    run_case(case, dtype, klass, ops)


@pytest.mark.parametrize("case,dtype,klass", params_of(R.SCN_CASES), ids=ids)
def test_narrow_output_two_sources(ops, case, dtype, klass):
    run_case(case, dtype, klass, ops)


@pytest.mark.parametrize("case,dtype,klass", params_of(R.STEM_CASES), ids=ids)
def test_stem(ops, case, dtype, klass):
    """Even widths: the persistent kernel; 1,19,67: the single-shot one.  The fourth input channel and the eighth tap column carry
    non-zero data against zero weights."""
    run_case(case, dtype, klass, ops)


# ---------------------------------------------------------------------------------------------------------------------------------
# second and third trip of the tile loop

@pytest.mark.parametrize("case,dtype,klass", params_of(R.TRIP_CASES), ids=ids)
def test_second_trip_of_the_tile_loop(ops, case, dtype, klass):
    """More tiles than persistent workgroups (asserted before the launch): the second half of the double buffer, the prefetch of the next
    tile and the idle DMA behind the last one, the lean kernel's hand-over of next-tile operands, the sums carried across tiles, the
    XCD-contiguous walk with ntiles & 7 != 0.  EXACT class: whole-tensor totals below 2^24 make every partition exact."""
    run_case(case, dtype, klass, ops)


# ---------------------------------------------------------------------------------------------------------------------------------
# the switches: read once per process

def child(select, **env):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, STP_SC_OPS_CHILD="1", **env)
    cmd = [sys.executable, "-m", "pytest", "-q", "-x", "-p", "no:cacheprovider", os.path.abspath(__file__), "-k", select]
    return subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300, cwd=root)


SC_SELECT = "(test_every_mode or test_summed or test_upsampled) and exact"
SELECT = {"STP_SC_LEAN": SC_SELECT, "STP_SC_STREAM": SC_SELECT, "STP_STEM_LEAN": "test_stem and exact"}


@pytest.mark.parametrize("switch", sorted(SELECT))
def test_switch_off_in_its_own_process(switch):
    """STP_SC_LEAN=0 (the generic streaming kernel serves everything), STP_SC_STREAM=0 (the single-shot conv_sc_kernel, one column per
    tile) and STP_STEM_LEAN=0 (the single-shot stem kernel): every exact comparison of the 1,21,67 / stem cases must still hold.  The
    child selects by test name and class; this test's own name matches neither, and a child never starts a child."""
    assert "STP_SC_OPS_CHILD" not in os.environ, "a child process selected the test that starts child processes"
    select = SELECT[switch]
    assert "switch" not in select
    r = child(select, **{switch: "0"})
    assert r.returncode == 0 and " passed" in r.stdout and "failed" not in r.stdout, switch + r.stdout[-3000:] + r.stderr[-3000:]


# ---------------------------------------------------------------------------------------------------------------------------------
# what the library refuses

@pytest.mark.parametrize("dtype", R.DTYPES)
def test_refusals(ops, dtype):
    """STP_E_BADARG, nothing launched: every pointer names one zeroed scratch buffer larger than any operand of these shapes."""
    from segmentation_training_pipeline_amd import _lib
    scratch = keep(torch.zeros(8 << 20, dtype=torch.uint8, device=DEV))
    names = "src0 src1 weight bias dst0 dst1 stats bnb_x bnb_mean bnb_rstd bnb_gamma bnb_beta pbn_mean pbn_rstd pbn_gamma pbn_beta"
    ptr = dict.fromkeys(names.split(), scratch.data_ptr())
    torch.cuda.synchronize()
    rcs = []
    for case, mode, over, what, eligible in R.REFUSALS:
        if dtype not in case.builds:
            continue
        P = R.fill_params(_lib.ConvParams(), case, mode, dtype, ptr, **over)
        assert bool(getattr(lib(), R.ELIGIBLE[case.kind])(C.byref(P))) == bool(eligible), what
        rcs.append((what, int(lib().stp_conv2d(C.byref(P), stream()))))
    assert rcs and all(rc == R.BADARG for _, rc in rcs), rcs
