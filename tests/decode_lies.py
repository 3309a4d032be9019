"""The lie matrix of the store decode's launch rule: size hints that drive every arm of it, and the arm each must select (decode_policy.hpp: policy_decode_plan).
Shared by tests/test_decode_planning_gpu.py (each arm is launched over real content) and tests/test_decode_policy_cpu.py (the rule alone, on the host)."""

TILED_VECTORS = 65600  # two segments of kSegmentMinVectors (host_ctx.hpp); more than the 32 768 the float stream shape and the forced read-ahead need

# name: (packed bits per value, exception bytes per vector, every rowgroup ALP_RD) -> the arm expected (double: vectors per workgroup, 256-entry stage, pad KiB)
LIES_F64 = {
    "all_0_bit":             ((1 / 128 / TILED_VECTORS, 0, False), (1, False, 14)),
    "narrow_2_bits":         ((2, 0, False), (2, False, 0)),
    "narrow_6_bits":         ((6, 0, False), (2, False, 0)),
    "narrow_with_exc":       ((6, 200, False), (2, False, 0)),
    "two_per_wg_capped":     ((12, 0, False), (2, False, 3)),
    "one_per_wg_6k":         ((20, 0, False), (1, False, 6)),
    "one_per_wg_uncapped":   ((32, 0, False), (1, False, 0)),
    "band_30_with_exc":      ((30, 200, False), (1, False, 6)),
    "band_38_with_exc":      ((38, 200, False), (1, False, 11)),
    "band_46_with_exc":      ((46, 200, False), (1, False, 14)),
    "band_38_no_exc":        ((38, 0, False), (1, False, 14)),
    "exception_heavy":       ((40, 1300, False), (1, True, 11)),
    "exception_heavy_26_bits": ((26, 1300, False), (1, True, 6)),
    "exception_heavy_all_rd": ((40, 1300, True), (1, False, 11)),
    "all_rd":                ((56, 0, True), (1, False, 11)),
}
# float: (vectors per workgroup or streamed shape)
LIES_F32 = {
    "all_0_bit":         ((1 / 128 / TILED_VECTORS, 0, False), 2),
    "narrow_2_bits":     ((2, 0, False), 27),
    "narrow_6_bits":     ((6, 0, False), 27),
    "narrow_8_bits":     ((8, 0, False), 27),
    "narrow_with_exc":   ((6, 120, False), 2),
    "wide":              ((20, 0, False), 2),
    "exception_heavy":   ((30, 1300, False), 2),
    "all_rd":            ((28, 0, True), 2),
}


def lie_hints(n, packed_bits, exc_bytes_per_vector, rd):
    """(packed_bytes_hint, exc_bytes_hint, alp_rd_rowgroups_hint) of a column of n vectors that tells this lie"""
    return max(1, int(packed_bits * 128 * n)), int(exc_bytes_per_vector * n), 1 + ((n + 99) // 100 if rd else 0)
