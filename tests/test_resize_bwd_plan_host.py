"""Host checks of the resize gradient's plan (csrc/resize_bwd.hip): stp_resize_bilinear_bwd_form launches nothing and looks
at its pointers only for null and alignment, so the library built on this host answers with fake ones (as tests/_wgrad_plan_dump.py
asks the weight-gradient planner).  The form each GPU case is meant to reach, the agreement of the form query with the workspace
query, the refusals, and what a misaligned dY does."""
import pytest

import _resize_bwd_cases as R

FAKE = 0x10000        # a 16-byte aligned address that is never read
HUGE = 1 << 40


@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
def test_every_gpu_case_reaches_the_form_it_names(dtype):
    for (n, h, w, c, ldo, coff, f), use_ws, forms in R.all_calls():
        wsb = R.workspace_bytes(n, h, w, c, f) if use_ws else 0
        got = R.form_of(FAKE, FAKE, n, h, w, c, f, ldo, coff, dtype, FAKE if wsb else None, wsb)
        assert got == R.want(forms, dtype), ((n, h, w, c, ldo, coff, f), use_ws, R.FORM_NAMES[got])
    reached = {R.want(forms, dtype) for _, _, forms in R.all_calls()}
    assert reached == set(range(7)) - ({R.TILE} if dtype == "fp32" else set())       # (the tile kernel is 16-bit only)


def grid():
    """The GPU cases, and around them channel counts of every vector width, slices, and factors on both sides of the tiny form's 8."""
    shapes = {s for s, _, _ in R.all_calls()}
    for n, h, w in ((1, 1, 1), (2, 3, 3), (1, 16, 8), (1, 17, 8), (1, 16, 9), (4, 24, 24), (1, 64, 64)):
        for c, ldo, coff in ((8, 8, 0), (4, 12, 4), (3, 3, 0), (6, 6, 0), (64, 64, 0), (100, 100, 0), (512, 1024, 512), (648, 712, 64)):
            for f in (1, 2, 3, 7, 8, 16, 48):
                if n * h * f * w * f * ldo <= 1 << 28:
                    shapes.add((n, h, w, c, ldo, coff, f))
    return sorted(shapes)


@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
def test_form_query_agrees_with_workspace_query(dtype):
    seen = set()
    for n, h, w, c, ldo, coff, f in grid():
        wsb = R.workspace_bytes(n, h, w, c, f)
        args = (FAKE, FAKE, n, h, w, c, f, ldo, coff, dtype)
        bare = R.form_of(*args, None, 0)
        assert bare not in (R.TINY, R.BLOCK_SPLIT)
        assert R.form_of(*args, None, HUGE) == bare and R.form_of(*args, FAKE, 0) == bare        # no pointer, no bytes: no workspace
        free = R.form_of(*args, FAKE, HUGE)
        if free in (R.TINY, R.BLOCK_SPLIT):
            assert wsb > 0
            assert R.form_of(*args, FAKE, wsb) == free          # the queried size is enough for the form an unbounded one gives
        else:
            assert free == bare
        if wsb == 0:
            assert free == bare
        seen.add(free)
    assert seen == set(range(7)) - ({R.TILE} if dtype == "fp32" else set())


def test_form_query_refusals():
    for (n, h, w, c, f, ldo, coff) in ((1, 4, 4, 4, 0, 4, 0), (1, 4, 4, 4, 2, 7, 4), (1, 4, 4, 4, 2, 8, -1), (1, 4, 4, 0, 2, 8, 0), (1, 0, 4, 4, 2, 8, 0)):
        assert R.form_of(FAKE, FAKE, n, h, w, c, f, ldo, coff, "fp32", None, 0) == R.BADARG
    assert R.form_of(None, FAKE, 1, 4, 4, 4, 2, 4, 0, "fp32", None, 0) == R.BADARG
    assert R.form_of(FAKE, None, 1, 4, 4, 4, 2, 4, 0, "fp32", None, 0) == R.BADARG
    assert R.form_of(FAKE, FAKE, 1, 4, 4, 4, 2, 4, 0, "fp32", None, 0) >= 0
    # the other build's 16-bit code
    assert R.form_of(FAKE, FAKE, 1, 4, 4, 8, 2, 8, 0, "bf16", None, 0) >= 0 and R.form_of(FAKE, FAKE, 1, 4, 4, 8, 2, 8, 0, "fp16", None, 0) >= 0
    lib16 = R._lib.load("fp16")
    assert int(lib16.stp_resize_bilinear_bwd_form(FAKE, FAKE, 1, 4, 4, 8, 2, 8, 0, R._lib.BF16, None, 0)) == R.BADARG


@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
def test_misaligned_dy_moves_a_tiny_or_rows_case_to_another_form(dtype):
    moved = 0
    for (n, h, w, c, ldo, coff, f), use_ws, forms in R.all_calls():
        if R.want(forms, dtype) not in (R.TINY, R.ROWS):
            continue
        wsb = R.workspace_bytes(n, h, w, c, f) if use_ws else 0
        got = R.form_of(FAKE + 8, FAKE, n, h, w, c, f, ldo, coff, dtype, FAKE if wsb else None, wsb)
        assert got >= 0 and got not in (R.TINY, R.ROWS, R.TILE), ((n, h, w, c, ldo, coff, f), got)
        moved += 1
    assert moved >= 8
