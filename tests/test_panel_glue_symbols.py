"""The panel-glue switch exists (no GPU needed: dlsym and attribute checks)."""


def test_panel_glue_switch_exported():
    import conflux_amd
    fn = conflux_amd.lib().conflux_lu_debug_set_panel_glue  # AttributeError
    assert fn.argtypes, "argtypes not declared in conflux_amd"
