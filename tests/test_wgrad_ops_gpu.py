"""GPU op tests of the weight-gradient kernels (csrc/conv_wgrad*.hip and the small-channel / stem kernels of conv_sc_wgrad.hip and
conv_sc_lean.hip), in fp32 and in both 16-bit builds.  Every entry point is called directly and compared with the float64 numpy
restatement of tests/_wgrad_reference.py - never with a second kernel, and with no tolerance scaled by a tensor's largest element or
taken from a kernel's output:

* EXACT cases: x integer in +-3, dy integer in +-2, a prior dW integer in +-1000.  tests/test_wgrad_reference_host.py asserts on these
  very inputs that every sum of absolute products stays below 2^24, so any order of fp32 additions over any number of slabs is exact:
  ``np.array_equal``.  A fused producer BatchNormalization runs with mean 0, rstd 1, gamma 1, beta 0 (the pre-activation is x exactly)
  over inputs that include -0.0, 6 and 7.
* ROUNDED cases: normal operands rounded to storage first; ``|got - ref| <= rounding_bound`` element by element, the bound being the
  worst case of any fp32 summation order over the element's own products (no storage term: dW is fp32).  With a fused
  BatchNormalization the reference is taken over the tensor stp_bn_apply wrote.

Every destination is pre-filled with NaN (or the known prior values when the launch accumulates) and carries 64 canary floats behind
it; every workspace - the group's workspace and device table too - is EXACTLY the queried size, NaN-filled, with a canary behind it;
the canaries are compared bit for bit after every launch; every launch is repeated and the bytes of dW compared; refusals are checked
on the return code, last, with nothing read afterwards.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import _wgrad_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
TD = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
BADARG = -1
CANARY_FLOATS = 64
CANARY_BITS = 0x5CA1AB1E
CLASSES = ["exact", "rounded"]


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
    torch.cuda.synchronize()
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


class Guarded(object):
    """``n`` fp32 elements of device memory with CANARY_FLOATS canary floats directly behind them."""

    def __init__(self, n):
        self.n = int(n)
        self.buf = keep(torch.empty(self.n + CANARY_FLOATS, dtype=torch.float32, device=DEV))
        self.data = self.buf[:self.n]
        self.canary = self.buf[self.n:].view(torch.int32)
        self.canary.fill_(CANARY_BITS)

    def ptr(self):
        return self.buf.data_ptr()

    def fill(self, values=None):
        """NaN, or the given prior contents."""
        if values is None:
            self.data.fill_(float("nan"))
        else:
            self.data.copy_(torch.from_numpy(np.ascontiguousarray(values, dtype=np.float32).reshape(-1)))

    def intact(self):
        torch.cuda.synchronize()
        return bool((self.canary == CANARY_BITS).all().item())

    def read(self):
        return host(self.data).copy()


class Layer(object):
    """One weight-gradient layer on the device: operands, guarded dW, and (for a launch of its own) the exactly sized workspace."""

    def __init__(self, case, dtype, d, act=None, fused=True, own_workspace=True):
        from segmentation_training_pipeline_amd import _lib
        self.case, self.dtype, self.d = case, dtype, d
        bn_on = case.bn is not None and fused
        src0 = dev(d["x0"], dtype) if (bn_on or act is None) else act      # a fused BatchNormalization reads the pre-activation tensor
        src1 = dev(d["x1"], dtype) if d["x1"] is not None else None
        dy = dev(d["dy"], dtype)
        self.bn = [f32(a) for a in d["bn"]] if bn_on else None
        self.shape = (case.co, case.kh, case.kw, case.c0 + case.c1)
        self.dw = Guarded(int(np.prod(self.shape)))
        self.P = R.fill_params(_lib.WgradParams(), case, dtype, src0.data_ptr(), dy.data_ptr(), self.dw.ptr(),
                               src1=src1.data_ptr() if src1 is not None else None, bn=[b.data_ptr() for b in self.bn] if bn_on else None)
        self.ws = None
        if own_workspace:
            self.ws_bytes = int(lib().stp_conv2d_wgrad_workspace_bytes(C.byref(self.P)))
            assert self.ws_bytes > 0 and self.ws_bytes % 4 == 0
            self.ws = Guarded(self.ws_bytes // 4)

    def stream(self):
        return torch.cuda.current_stream().cuda_stream

    def launch(self, variant=None, prev=None):
        """variant None: stp_conv2d_wgrad; 0-4: stp_conv2d_wgrad_partial + _reduce.  -> dW as the launch left it (canaries checked)."""
        self.P.accumulate = 0 if prev is None else 1
        self.dw.fill(prev)
        self.ws.fill()
        if variant is None:
            rc = lib().stp_conv2d_wgrad(C.byref(self.P), self.ws.ptr(), self.ws_bytes, self.stream())
            assert rc == 0, "stp_conv2d_wgrad: %d" % rc
        else:
            rc = lib().stp_conv2d_wgrad_partial(C.byref(self.P), self.ws.ptr(), self.ws_bytes, variant, self.stream())
            assert rc == 0, "stp_conv2d_wgrad_partial(variant %d): %d" % (variant, rc)
            rc = lib().stp_conv2d_wgrad_reduce(C.byref(self.P), self.ws.ptr(), variant, self.stream())
            assert rc == 0, "stp_conv2d_wgrad_reduce(variant %d): %d" % (variant, rc)
        out = self.dw.read()
        assert self.ws.intact(), "variant %s wrote behind the %d bytes stp_conv2d_wgrad_workspace_bytes asked for" % (variant, self.ws_bytes)
        assert self.dw.intact(), "variant %s wrote behind dW" % variant
        return out

    def twice(self, variant=None, prev=None):
        a, b = self.launch(variant, prev), self.launch(variant, prev)
        assert a.tobytes() == b.tobytes(), "variant %s: a second identical launch gave different bytes" % variant
        return a.reshape(self.shape)

    def refused(self, variant):
        """Return code of a partial launch that must not start (nothing is synchronised or read afterwards)."""
        return int(lib().stp_conv2d_wgrad_partial(C.byref(self.P), self.ws.ptr(), self.ws_bytes, variant, self.stream()))


def compare(klass, got, d, what, accumulated=False, unpad=None):
    """EXACT: equal as numbers, nothing left unwritten.  ROUNDED: within the element's own rounding bound."""
    ref = d["dw_acc"] if accumulated else d["dw"]
    ab, nt, prev = d["abs"], d["nt"], (d["prev"] if accumulated else None)
    if unpad is not None:
        ref, ab, nt, prev = unpad(ref), unpad(ab), unpad(nt), (unpad(prev) if prev is not None else None)
    assert got.shape == ref.shape
    assert not np.isnan(got).any(), "%s: %d elements were not written" % (what, int(np.isnan(got).sum()))
    if klass == "exact":
        bad = got.astype(np.float64) != ref
        assert not bad.any(), "%s: %d of %d elements differ from the exact sum, first at %s: %r against %r" % (
            what, int(bad.sum()), bad.size, tuple(np.argwhere(bad)[0]), float(got[bad][0]), float(ref[bad][0]))
        return
    bound = R.rounding_bound(nt, ab, prev)
    err = np.abs(got.astype(np.float64) - ref)
    ratio = float((err / np.maximum(bound, 1e-300)).max())
    print("WGRAD_RATIO %s: max error / bound = %.4f" % (what, ratio))
    bad = err > bound
    assert not bad.any(), "%s: %d of %d elements outside the bound, worst %.3g against %.3g" % (
        what, int(bad.sum()), bad.size, float(err[bad].max()), float(bound[bad][err[bad].argmax()]))


def inputs(ops, case, dtype, klass):
    """-> (d with the float64 reference, act) ; act = the device tensor stp_bn_apply wrote (ROUNDED class with a BatchNormalization)."""
    if klass == "exact":
        return R.exact_case(case), None
    if case.bn is None:
        return R.rounded_case(case, dtype), None
    d = R.rounded_inputs(case, dtype)
    pre = dev(d["x0"], dtype)
    act = keep(torch.empty_like(pre))
    mean, rstd, gamma, beta = [f32(a) for a in d["bn"]]
    ops.bn_apply(pre, act, case.n * case.h * case.w, case.c0, case.c0, mean, rstd, gamma, beta, relu=case.bn)
    return R.rounded_reference(case, d, act=host(act)), act


def unpad_launch(ops, layer, padded):
    """stp_weight_grad_unpad behind the stem's padded gradient -> [Cout][7][7][3], guarded."""
    co = layer.case.co
    src = f32(padded.reshape(-1))
    g = Guarded(co * 7 * 7 * 3)
    g.fill()
    ops.weight_grad_unpad(src, g.buf, co, 7, 7, 3, 8, 4)
    out = g.read().reshape(co, 7, 7, 3)
    assert g.intact(), "stp_weight_grad_unpad wrote behind its destination"
    return out


def check_layer(ops, layer, klass, got, what, accumulated=False):
    if layer.case.stem:
        compare(klass, unpad_launch(ops, layer, got), layer.d, what, accumulated, unpad=R.unpad_stem)
    else:
        compare(klass, got, layer.d, what, accumulated)


def ids(v):
    return v if isinstance(v, str) else "%s-%s" % (v.family, v.name)


def params_of(cases, classes=CLASSES):
    return [(c, dt, k) for c in cases for dt in R.dtypes_of(c) for k in classes]


# ---------------------------------------------------------------------------------------------------------------------------------
# the pixel-reduction GEMM: four tiles x three staging variants, uniform-row / general addressing, split-K slabs + reduce, the C4 stem

@pytest.mark.parametrize("case,dtype,klass", params_of(R.GEMM_CASES), ids=ids)
def test_gemm_family(ops, case, dtype, klass):
    d, _ = inputs(ops, case, dtype, klass)
    L = Layer(case, dtype, d)
    tag = "gemm/%s/%s" % (case.name, dtype)
    assert int(lib().stp_conv2d_wgrad_kernel_id(C.byref(L.P))) == R.expected_kernel_id(case, dtype)
    check_layer(ops, L, klass, L.twice(), tag + " auto")
    check_layer(ops, L, klass, L.twice(prev=d["prev"]), tag + " auto accumulate", accumulated=True)
    row = R.row_eligible(case, dtype)
    for variant in (1, 2, 3) + ((4,) if row else ()):
        check_layer(ops, L, klass, L.twice(variant), "%s variant %d" % (tag, variant))
    check_layer(ops, L, klass, L.twice(2, prev=d["prev"]), tag + " variant 2 accumulate", accumulated=True)
    if not row:
        assert L.refused(4) == BADARG


# ---------------------------------------------------------------------------------------------------------------------------------
# the persistent small-channel kernel (kernel_id 1), its two-source form, its fused BatchNormalization, the lean stem kernel

def run_small_channel(ops, case, dtype, klass):
    d, act = inputs(ops, case, dtype, klass)
    L = Layer(case, dtype, d, act=act)
    tag = "sc/%s/%s" % (case.name, dtype)
    assert int(lib().stp_conv2d_wgrad_kernel_id(C.byref(L.P))) == 1
    if case is R.SC_MULTI_TRIP:      # one slab per persistent workgroup: fewer workgroups than tiles
        assert L.ws_bytes // (L.dw.n * 4) < R.sc_tiles(case)
    check_layer(ops, L, klass, L.twice(), tag + " auto")
    check_layer(ops, L, klass, L.twice(prev=d["prev"]), tag + " auto accumulate", accumulated=True)
    if case.bn is not None:
        assert L.refused(1) == BADARG                 # the GEMM variants have no fused producer BatchNormalization


@pytest.mark.parametrize("case,dtype,klass", params_of(R.SC_CASES), ids=ids)
def test_small_channel_kernel(ops, case, dtype, klass):
    run_small_channel(ops, case, dtype, klass)


@pytest.mark.parametrize("dtype", R.DTYPES)
def test_small_channel_kernel_second_trip_of_the_tile_loop(ops, dtype):
    """2 x 258 x 500 pixels = 1056 tiles of 8 x 32 against at most 1024 (fp32: 512) persistent workgroups: some take a second tile.
    Exact class only: 258 000 pixel products of at most 6 each stay below 1.55e6."""
    run_small_channel(ops, R.SC_MULTI_TRIP, dtype, "exact")


# ---------------------------------------------------------------------------------------------------------------------------------
# the row-of-taps kernel (variant 4; automatic in the 16-bit builds): two tiles, splits, two sources, a fused BatchNormalization

@pytest.mark.parametrize("case,dtype,klass", params_of(R.ROW_CASES), ids=ids)
def test_row_of_taps_kernel(ops, case, dtype, klass):
    d, act = inputs(ops, case, dtype, klass)
    L = Layer(case, dtype, d, act=act)
    tag = "row/%s/%s" % (case.name, dtype)
    assert R.row_eligible(case, dtype)
    assert int(lib().stp_conv2d_wgrad_kernel_id(C.byref(L.P))) == R.expected_kernel_id(case, dtype)
    check_layer(ops, L, klass, L.twice(4), tag + " variant 4")
    check_layer(ops, L, klass, L.twice(4, prev=d["prev"]), tag + " variant 4 accumulate", accumulated=True)
    if case.bn is None or not case.splits:
        check_layer(ops, L, klass, L.twice(), tag + " auto")
        check_layer(ops, L, klass, L.twice(prev=d["prev"]), tag + " auto accumulate", accumulated=True)
    if case.bn is not None:
        assert L.refused(2) == BADARG                 # the GEMM variants have no fused producer BatchNormalization


# ---------------------------------------------------------------------------------------------------------------------------------
# the grouped launch (row-of-taps and all-taps tiles): one partial + one reduce launch over a descriptor table

class Group(object):
    """stp_wgrad_group_* over ``layers``: the table on the device and the workspace are exactly the queried bytes, both guarded."""

    def __init__(self, ops, layers):
        self.layers = layers
        built = ops.WgradGroup([l.P for l in layers])      # queries the table and workspace sizes and builds the host table
        self.built, self.host, self.header = built, built.host, built.header
        self.tb, self.wsb = len(built.host), built.ws.numel() * 4
        assert built.dev.numel() == self.tb and self.wsb > 0
        self.table = keep(torch.full((self.tb + 256,), 0xA5, dtype=torch.uint8, device=DEV))
        self.table[:self.tb].copy_(torch.frombuffer(bytearray(bytes(self.host)), dtype=torch.uint8))
        self.ws = Guarded(self.wsb // 4)

    def launch(self, prevs=None):
        st = torch.cuda.current_stream().cuda_stream
        for i, l in enumerate(self.layers):
            l.dw.fill(None if prevs is None else prevs[i])
        self.ws.fill()
        rc = int(lib().stp_wgrad_group_partial(C.addressof(self.host), self.table.data_ptr(), self.ws.ptr(), self.wsb, st))
        assert rc == 0, "stp_wgrad_group_partial: %d" % rc
        rc = int(lib().stp_wgrad_group_reduce(C.addressof(self.host), self.table.data_ptr(), self.ws.ptr(), st))
        assert rc == 0, "stp_wgrad_group_reduce: %d" % rc
        outs = [l.dw.read() for l in self.layers]
        assert self.ws.intact(), "the group wrote behind the %d bytes of workspace its size query asked for" % self.wsb
        assert bool((self.table[self.tb:] == 0xA5).all().item()) and bytes(self.table[:self.tb].cpu().numpy()) == bytes(self.host), "the device table changed"
        for l in self.layers:
            assert l.dw.intact(), "the group wrote behind the dW of layer %s" % l.case.name
        return outs

    def twice(self, prevs=None):
        a, b = self.launch(prevs), self.launch(prevs)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)), "a second identical group launch gave different bytes"
        return [x.reshape(l.shape) for x, l in zip(a, self.layers)]


def run_group(ops, group, dtype, klass, fused_index=None):
    cases = [R.group_case(group, i, bn=(1 + i % 2) if i == fused_index else None) for i in range(len(R.GROUPS[group]))]
    layers = []
    for c in cases:
        d, act = inputs(ops, c, dtype, klass)
        layers.append(Layer(c, dtype, d, act=act, own_workspace=False))
    assert [int(lib().stp_wgrad_group_class(C.byref(l.P))) for l in layers] == [R.GROUP_CLASS[group]] * len(layers)
    G = Group(ops, layers)
    assert G.header[1] == R.GROUP_CLASS[group] and G.header[2] == len(layers) and G.header[14] == (0 if fused_index is None else 1)
    tag = "group/%s/%s%s" % (group, dtype, "" if fused_index is None else "/bn")
    for got, l in zip(G.twice(), layers):
        compare(klass, got, l.d, "%s %s" % (tag, l.case.name))
    for l in layers:
        l.P.accumulate = 1                               # the table records the flag when it is built
    GA = Group(ops, layers)
    for got, l in zip(GA.twice([l.d["prev"] for l in layers]), layers):
        compare(klass, got, l.d, "%s %s accumulate" % (tag, l.case.name), accumulated=True)


@pytest.mark.parametrize("klass", CLASSES)
@pytest.mark.parametrize("dtype", R.H16)
@pytest.mark.parametrize("group", sorted(R.GROUPS))
def test_grouped_launch(ops, group, dtype, klass):
    run_group(ops, group, dtype, klass)


@pytest.mark.parametrize("klass", CLASSES)
@pytest.mark.parametrize("dtype", R.H16)
@pytest.mark.parametrize("group", ["class128", "class64", "class32"])
def test_grouped_launch_with_one_fused_batchnorm_layer(ops, group, dtype, klass):
    """One layer of the group reads its source through a fused producer BatchNormalization (ReLU / ReLU6), the others do not."""
    direct = [i for i, s in enumerate(R.GROUPS[group]) if s[4] == 0]
    run_group(ops, group, dtype, klass, fused_index=direct[len(direct) // 2])


# ---------------------------------------------------------------------------------------------------------------------------------
# the batched reduce of lone layers

@pytest.mark.parametrize("dtype", R.DTYPES)
def test_batched_reduce_exact_and_equal_to_the_per_layer_reduce(ops, dtype):
    """stp_wgrad_reduce_batched over the five lone layers, EXACT class: equal to the float64 sums, and the per-layer
    stp_conv2d_wgrad_reduce of the same slabs - another order of the same exact additions - EQUAL to it, not merely close."""
    n = len(R.LONE_LAYERS)
    layers = [Layer(R.lone_case(i), dtype, R.exact_case(R.lone_case(i))) for i in range(n)]
    db = int(lib().stp_wgrad_reduce_desc_bytes())
    st = torch.cuda.current_stream().cuda_stream

    def batched(accumulate):
        table = (C.c_char * (db * n))()
        counts = []
        for i, l in enumerate(layers):
            l.P.accumulate = accumulate
            l.dw.fill(l.d["prev"] if accumulate else None)
            l.ws.fill()
            counts.append(int(lib().stp_wgrad_reduce_desc_fill(C.addressof(table), i, C.byref(l.P), l.ws.ptr())))
            assert counts[-1] == l.dw.n
        tdev = keep(torch.full((db * n + 256,), 0xA5, dtype=torch.uint8, device=DEV))
        tdev[:db * n].copy_(torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8))
        for l in layers:
            assert int(lib().stp_conv2d_wgrad_partial(C.byref(l.P), l.ws.ptr(), l.ws_bytes, 0, st)) == 0
        assert int(lib().stp_wgrad_reduce_batched(tdev.data_ptr(), n, max(counts), st)) == 0
        outs = [l.dw.read() for l in layers]
        for l in layers:
            assert l.ws.intact() and l.dw.intact(), "lone layer %s: a canary changed" % l.case.name
        assert bool((tdev[db * n:] == 0xA5).all().item())
        return outs

    for accumulate in (0, 1):
        first, again = batched(accumulate), batched(accumulate)
        for l, a, b in zip(layers, first, again):
            assert a.tobytes() == b.tobytes()
            compare("exact", a.reshape(l.shape), l.d, "lone/%s/%s batched" % (l.case.name, dtype), accumulated=bool(accumulate))
            l.dw.fill(l.d["prev"] if accumulate else None)      # the per-layer reduce of the slabs the batched launch just read
            assert int(lib().stp_conv2d_wgrad_reduce(C.byref(l.P), l.ws.ptr(), 0, st)) == 0
            per_layer = l.dw.read()
            assert l.ws.intact() and l.dw.intact()
            assert np.array_equal(per_layer, b), "lone layer %s: the per-layer reduce differs from the batched one" % l.case.name
