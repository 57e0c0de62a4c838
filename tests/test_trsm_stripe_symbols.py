"""The stripe-solve switch and its debug entries exist (no GPU needed: dlsym
and attribute checks)."""
import pytest


@pytest.mark.parametrize("name", ["conflux_lu_debug_set_trsm_stripe",
                                  "conflux_lu_debug_trsm_ld"])
def test_trsm_stripe_entries_exported(name):
    import conflux_amd
    fn = getattr(conflux_amd.lib(), name)  # AttributeError if not exported
    assert fn.argtypes, "argtypes not declared in conflux_amd"


def test_trsm_stripe_width_exported():
    import conflux_amd
    fn = conflux_amd.lib().conflux_lu_debug_trsm_stripe_width
    assert fn.argtypes is not None and len(fn.argtypes) == 0
