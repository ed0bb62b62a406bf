"""No-GPU checks of the argument validation that runs before an entry point's first HIP call: the one switch on the
point type (csrc/fq2.cuh by_point_type) in every entry that takes a `type`, the pair-count check of the MSM entries,
the `part` of the accumulate stage, and the version of the C ABI.  Pointers are dummy non-null values: nothing may
dereference them, on the host or on a device."""
import ctypes

import pytest

INVALID = -1
P, Q, R = 0x10000, 0x20000, 0x30000     # distinct, 4-byte aligned, never dereferenced
BIG = 1 << 40


@pytest.fixture(scope="module")
def L():
    from octopuszk_amd import build, lib
    build.build(verbose=False)
    return lib.load()


def _entries(L, n, type_, part=0):
    """name -> call of every `*_dev` entry that dispatches on `type`, with otherwise acceptable arguments"""
    one = (ctypes.c_uint8 * 32)(1)      # host memory: the scalar 1 / the root of unity of order 1
    sizes = [ctypes.c_size_t() for _ in range(3)]
    fields = (ctypes.c_int64 * 22)()
    return {
        "ozk_var_msm_stage_bytes": lambda: L.ozk_var_msm_stage_bytes(n, type_, *[ctypes.byref(s) for s in sizes]),
        "ozk_var_msm_stage_layout": lambda: L.ozk_var_msm_stage_layout(n, type_, 0, fields, 22),
        "ozk_var_msm_dev": lambda: L.ozk_var_msm_dev(P, Q, n, type_, R, R, BIG, None),
        "ozk_var_msm_prepared_dev": lambda: L.ozk_var_msm_prepared_dev(P, Q, n, type_, R, R, BIG, None),
        "ozk_var_msm_prepare_dev": lambda: L.ozk_var_msm_prepare_dev(P, n, type_, R, BIG, None),
        "ozk_var_msm_head_dev": lambda: L.ozk_var_msm_head_dev(P, 0, Q, n, type_, R, BIG, R, BIG, None, None),
        "ozk_var_msm_tail_dev": lambda: L.ozk_var_msm_tail_dev(n, type_, P, BIG, R, None, None, 0),
        "ozk_var_msm_sort_dev": lambda: L.ozk_var_msm_sort_dev(P, 0, Q, n, type_, R, BIG, R, BIG, None),
        "ozk_var_msm_accum_dev": lambda: L.ozk_var_msm_accum_dev(None, n, type_, P, BIG, Q, BIG, R, BIG, None, part),
        "ozk_points_sum_dev": lambda: L.ozk_points_sum_dev(P, n, type_, R, None),
        "ozk_points_decompress_dev": lambda: L.ozk_points_decompress_dev(P, n, type_, 0, Q, R, None),
        "ozk_points_decompress_prepared_dev":
            lambda: L.ozk_points_decompress_prepared_dev(P, n, type_, Q, BIG, R, 0, None),
        "ozk_points_compress_dev": lambda: L.ozk_points_compress_dev(P, n, type_, 0, Q, None),
        "ozk_points_scale_dev": lambda: L.ozk_points_scale_dev(P, n, type_, one, Q, None),
        "ozk_ec_fft_dev": lambda: L.ozk_ec_fft_dev(P, n, type_, one, 0, Q, R, BIG, None),
        "ozk_sparse_mat_points_dev":
            lambda: L.ozk_sparse_mat_points_dev(P, P, None, Q, n, type_, None, 0, R, None, 0, None),
        "ozk_points_add_dev": lambda: L.ozk_points_add_dev(P, Q, n, type_, 0, R, None),
    }


MSM_ENTRIES = ["ozk_var_msm_dev", "ozk_var_msm_prepared_dev", "ozk_var_msm_prepare_dev", "ozk_var_msm_head_dev",
               "ozk_var_msm_tail_dev", "ozk_var_msm_sort_dev", "ozk_var_msm_accum_dev"]


def test_version_is_two(L):
    assert L.ozk_version() == 2


@pytest.mark.parametrize("type_", [0, 3])
def test_unknown_point_type_is_rejected_without_a_device(L, type_):
    for query in (L.ozk_var_msm_workspace_bytes, L.ozk_var_msm_head_workspace_bytes, L.ozk_var_msm_tail_bytes,
                  L.ozk_var_msm_prepared_bytes, L.ozk_ec_fft_workspace_bytes, L.ozk_sparse_mat_points_workspace_bytes):
        assert query(1, type_) == 0
    for name, call in _entries(L, 1, type_).items():
        assert call() == INVALID, name
        assert b"unknown point type %d" % type_ in L.ozk_last_error(), (name, L.ozk_last_error())


@pytest.mark.parametrize("n", [0, (1 << 24) + 1])
def test_pair_count_out_of_range_is_rejected_without_a_device(L, n):
    entries = _entries(L, n, 1)
    for name in MSM_ENTRIES:
        assert entries[name]() == INVALID, name
        assert b"batch_size %d out of range [1, 2^24]" % n in L.ozk_last_error(), (name, L.ozk_last_error())


@pytest.mark.parametrize("part", [-1, 3])
def test_unknown_accumulate_part_is_rejected_without_a_device(L, part):
    assert _entries(L, 1, 1, part)["ozk_var_msm_accum_dev"]() == INVALID
    assert b"part %d is not 0 (all), 1 (level 1) or 2 (rest)" % part in L.ozk_last_error()


def test_null_pointers_are_rejected_before_the_type(L):
    assert L.ozk_var_msm_head_dev(None, 0, Q, 1, 3, R, BIG, R, BIG, None, None) == INVALID
    assert b"null pointer" in L.ozk_last_error()
    assert L.ozk_var_msm_tail_dev(1, 3, None, BIG, R, None, None, 0) == INVALID
    assert b"null pointer" in L.ozk_last_error()
