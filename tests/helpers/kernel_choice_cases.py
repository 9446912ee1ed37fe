"""Small plans that reach every covariance and power kernel kind (csrc/kernel_choice.h) at the smallest shapes that still do
and still have a ragged edge: frames that are no multiple of any step, bins that fill no workgroup.  Shared by
tests/test_kernel_choice_gpu.py and tools/ab_plan_bits.py."""

# (T, F, M, K, mode, cov_quad, cov_hmfma, float32 partials, covariance kind, power kind)
PLAN_CASES = [
    (70, 5, 3, 2, "fast", True, True, False, "Lane", "Lane"),
    (70, 5, 7, 3, "fast", True, True, False, "Lane", "Lane"),
    (70, 5, 8, 2, "fast", True, True, False, "Lane", "Lane"),
    (70, 5, 4, 2, "precise", True, True, False, "Lane", "Lane"),
    (70, 33, 8, 3, "fast", True, True, False, "Pair32", "Lane"),
    (70, 33, 8, 3, "mixed", True, True, False, "Pair32", "Lane"),
    (70, 33, 8, 2, "precise", True, True, False, "Pair64", "Lane"),
    (70, 3, 16, 2, "mixed", True, True, False, "Quad", "Lane"),
    (70, 3, 16, 2, "fast", True, True, False, "Quad", "Lane"),
    (70, 3, 11, 2, "fast", True, True, False, "Quad", "Lane"),
    (70, 3, 16, 6, "fast", True, True, False, "Half16", "Mfma"),
    (70, 3, 13, 8, "mixed", True, True, False, "Half16", "Mfma"),
    (70, 3, 16, 16, "fast", True, False, False, "Half16", "Mfma"),
    (70, 3, 16, 16, "fast", True, True, False, "Hmfma", "Mfma"),
    (70, 3, 16, 16, "fast", True, True, True, "Hmfma", "Mfma"),
    (70, 3, 10, 9, "mixed", True, True, False, "Hmfma", "Mfma"),
    (70, 3, 15, 15, "fast", True, True, False, "Hmfma", "Mfma"),
    (70, 3, 12, 12, "mixed", True, True, False, "Hmfma", "Mfma"),
    (70, 3, 16, 4, "precise", True, True, False, "Half16F64", "Lane"),
    (70, 3, 14, 8, "precise", True, True, False, "Half16F64", "Mfma"),
    (70, 3, 16, 16, "precise", True, True, False, "Hmfma64", "Mfma"),
    (70, 3, 15, 15, "precise", True, True, False, "Hmfma64", "Mfma"),
    (70, 3, 16, 2, "precise", True, True, False, "Mfma", "Lane"),
    (70, 3, 9, 3, "fast", False, True, False, "Mfma", "Lane"),
    (70, 3, 17, 3, "fast", True, True, False, "Wide", "Wide"),
    (40, 3, 24, 24, "mixed", True, True, False, "Wide", "Wide"),
    (48, 40, 16, 8, "mixed", True, True, False, "Half16", "Mfma"),
    (48, 65, 16, 16, "mixed", True, True, False, "Hmfma", "Lds"),
]
# one-source plans for an OGIVE chunk, one per kind a single source can reach (17..32 channels: OGIVE does not take them)
OGIVE_CASES = [
    (70, 5, 3, 1, "fast", "Lane"),
    (70, 33, 8, 1, "precise", "Pair64"),
    (70, 3, 16, 1, "mixed", "Quad"),
    (70, 3, 16, 1, "precise", "Mfma"),
]
QUAD_GOVERNED = ("Quad", "Half16", "Hmfma", "Half16F64", "Hmfma64")


def case_id(c):
    T, F, M, K, mode, quad, hm, p32 = c[:8]
    return f"T{T}F{F}M{M}K{K}-{mode}" + ("" if quad else "-noquad") + ("" if hm else "-nohmfma") + ("-part32" if p32 else "")
