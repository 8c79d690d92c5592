"""The cases of the bilinear resize gradient (csrc/resize_bwd.hip) with the form each is meant to reach, shared by the GPU tests of
tests/test_ops_gpu.py, which assert the form with the very arguments of the launch, and by tests/test_resize_bwd_plan_host.py, which
asks the same questions with fake pointers on a host without a GPU.  The forms were read from a kernel trace of the launches
(DESIGN.md 4.8), not from the query."""
from segmentation_training_pipeline_amd import _lib

# STP_RESIZE_BWD_* of include/stp_hip.h
GATHER, SLICE_COPY, TINY, ROWS, TILE, BLOCK, BLOCK_SPLIT = range(7)
FORM_NAMES = ["GATHER", "SLICE_COPY", "TINY", "ROWS", "TILE", "BLOCK", "BLOCK_SPLIT"]
BADARG = -1
DT = {"fp32": _lib.F32, "bf16": _lib.BF16, "fp16": _lib.F16}


def form_of(dy, dx, n, h, w, c, f, ldo, coff, dtype, ws, wsb):
    """stp_resize_bilinear_bwd_form of the library that serves ``dtype`` ("fp32" / "bf16" / "fp16"); pointers are integers or None."""
    lib = _lib.load("fp16" if dtype == "fp16" else "bf16")
    return int(lib.stp_resize_bilinear_bwd_form(dy, dx, n, h, w, c, f, ldo, coff, DT[dtype], ws, wsb))


def workspace_bytes(n, h, w, c, f):
    return int(_lib.load("bf16").stp_resize_bilinear_bwd_workspace_bytes(n, h, w, c, f))


def want(forms, dtype):
    """``forms`` = (form in fp32, form in either 16-bit storage)."""
    return forms[0] if dtype == "fp32" else forms[1]


# test_bilinear_resize_gradient_of_class_logits_and_of_an_unresized_slice: ((n, h, w, c, ldo, coff, factor), forms with the queried
# workspace, forms of a second run without a workspace or None)
SLICE_CASES = [
    # class logits: output rows streamed through LDS
    ((2, 12, 24, 24, 24, 0, 8), (ROWS, ROWS), None), ((1, 16, 64, 8, 8, 0, 4), (ROWS, ROWS), None), ((2, 6, 10, 8, 24, 8, 2), (ROWS, ROWS), None),
    ((1, 9, 33, 16, 16, 0, 8), (ROWS, ROWS), None),
    # factor 1 = a channel slice copied / added back
    ((2, 5, 7, 16, 48, 16, 1), (SLICE_COPY, SLICE_COPY), None), ((1, 8, 8, 128, 320, 64, 1), (SLICE_COPY, SLICE_COPY), None),
    # tiny maps, large factors, a slice of a wide tensor (PSPNet's pyramid levels): the separable two-pass form
    ((2, 1, 1, 128, 320, 64, 32), (TINY, TINY), None), ((1, 2, 2, 512, 1024, 512, 16), (TINY, TINY), None),
    ((2, 3, 3, 64, 192, 128, 24), (TINY, TINY), None), ((1, 6, 6, 256, 256, 0, 8), (TINY, TINY), None),
    # wide slices of a concatenation (FPN's pyramid levels: round 6, resize_bilinear_bwd_tile_kernel): two channel chunks, ragged
    # column segments, an odd row count (a row pair with one row), factors 8, 4 and 2
    ((1, 18, 20, 128, 512, 128, 8), (BLOCK, TILE), None), ((2, 17, 33, 64, 192, 64, 4), (BLOCK, TILE), None),
    ((1, 40, 36, 128, 512, 384, 2), (BLOCK, TILE), None),
    # narrow unsliced maps by a factor of 16 and of 3: their output rows fit the LDS buffer, so the row kernel takes them first
    ((1, 17, 3, 32, 32, 0, 16), (ROWS, ROWS), None), ((1, 20, 20, 48, 48, 0, 3), (ROWS, ROWS), None),
    # ... the same maps as slices whose output rows exceed 40 KB: the tile kernel with factors 16 and 3 in 16-bit storage
    ((1, 17, 3, 32, 512, 128, 16), (BLOCK_SPLIT, TILE), None), ((1, 20, 20, 48, 384, 96, 3), (BLOCK, TILE), None),
    # the workgroup-per-pixel kernel split over the workspace (few pixels, many taps) and, without a workspace, in one pass: a sliced fp32
    # map with two vector lanes (in 16-bit storage its rows fit the row kernel), 648 channels on two pixels in 16 (fp32) and 32 (16-bit)
    # splits, and 648 channels as a slice
    ((1, 2, 9, 8, 72, 64, 16), (BLOCK_SPLIT, ROWS), (BLOCK, ROWS)), ((1, 1, 2, 648, 648, 0, 16), (BLOCK_SPLIT, BLOCK_SPLIT), (BLOCK, BLOCK)),
    ((1, 2, 2, 648, 712, 64, 16), (BLOCK_SPLIT, BLOCK_SPLIT), (BLOCK, BLOCK)),
    # a tiny map without its workspace: the next form that accepts it
    ((1, 1, 5, 128, 192, 64, 16), (TINY, TINY), (BLOCK, ROWS)),
]

# test_tf1_bilinear_resize_into_channel_slice_and_gradient: (n, h, w, c, ldo, coff) = (2, 5, 7, 8, 24, 8), no workspace; factor -> forms
TF1_SHAPE = (2, 5, 7, 8, 24, 8)
TF1_FORMS = {1: (SLICE_COPY, SLICE_COPY), 2: (ROWS, ROWS), 4: (ROWS, ROWS), 8: (ROWS, ROWS)}

# test_pyramid_pooling_geometry_resize_and_pool: n = 2, unsliced; (h, w, factor, c) -> (forms with the queried workspace, forms without)
GEOM_FORMS = {
    (1, 1, 24, 320): ((ROWS, ROWS), (ROWS, ROWS)), (2, 2, 12, 72): ((ROWS, ROWS), (ROWS, ROWS)), (3, 3, 8, 40): ((ROWS, ROWS), (ROWS, ROWS)),
    (6, 6, 4, 24): ((ROWS, ROWS), (ROWS, ROWS)), (5, 7, 8, 20): ((ROWS, BLOCK), (ROWS, BLOCK)), (3, 2, 6, 3): ((GATHER, GATHER), (GATHER, GATHER)),
    (12, 12, 8, 24): ((ROWS, ROWS), (ROWS, ROWS)), (16, 16, 4, 8): ((ROWS, ROWS), (ROWS, ROWS)), (5, 7, 2, 8): ((ROWS, ROWS), (ROWS, ROWS)),
    (9, 3, 3, 16): ((ROWS, ROWS), (ROWS, ROWS)),
}


def all_calls():
    """Every (shape, workspace used, forms) the three GPU tests launch: ((n, h, w, c, ldo, coff, f), with workspace?, forms)."""
    out = []
    for shape, forms, bare in SLICE_CASES:
        out.append((shape, True, forms))
        if bare is not None:
            out.append((shape, False, bare))
    n, h, w, c, ldo, coff = TF1_SHAPE
    for f, forms in sorted(TF1_FORMS.items()):
        out.append(((n, h, w, c, ldo, coff, f), False, forms))
    for (h, w, f, c), (with_ws, bare) in sorted(GEOM_FORMS.items()):
        out.append(((2, h, w, c, c, 0, f), True, with_ws))
        out.append(((2, h, w, c, c, 0, f), False, bare))
    return out
