"""The kernel-pin debug entries exist and have argtypes (no GPU needed: dlsym
and attribute checks)."""
import pytest

ENTRIES = {
    "conflux_lu_debug_dgemm_ex": 12,
    "conflux_lu_debug_set_gemm_strip": 1,
    "conflux_lu_debug_set_gemm_ntc": 1,
    "conflux_lu_debug_dgemm_nt": 17,
    "conflux_lu_debug_potrf32": 4,
    "conflux_lu_debug_getrf32_nopiv": 4,
    "conflux_lu_debug_trsm32": 7,
    "conflux_lu_debug_potrf_tile": 4,
    "conflux_lu_debug_poke_factor": 4,
}


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_kernel_pin_entries_exported(name):
    import conflux_amd
    fn = getattr(conflux_amd.lib(), name)  # AttributeError if not exported
    assert fn.argtypes and len(fn.argtypes) == ENTRIES[name], \
        "argtypes not declared in conflux_amd"


def test_plain_dgemm_entry_kept():
    import conflux_amd
    assert len(conflux_amd.lib().conflux_lu_debug_dgemm.argtypes) == 6
