"""The leaf-kernel switches exist and round-trip (no GPU needed: the setters
only touch process-global modes)."""
import ctypes


def _lib():
    import conflux_amd
    return conflux_amd.lib()


def test_panel_reg_switches_exported():
    lib = _lib()
    for name in ("conflux_lu_debug_set_panel_reg",
                 "conflux_lu_debug_set_panel_publish",
                 "conflux_lu_debug_set_panel_phase_stats",
                 "conflux_lu_debug_panel_phase_stats"):
        fn = getattr(lib, name)  # AttributeError when missing
        assert fn.argtypes, f"argtypes of {name} not declared in conflux_amd"


def test_panel_reg_switches_round_trip():
    lib = _lib()
    for fn in (lib.conflux_lu_debug_set_panel_reg,
               lib.conflux_lu_debug_set_panel_publish,
               lib.conflux_lu_debug_set_panel_phase_stats):
        prev = fn(0)
        try:
            assert prev in (0, 1)
            assert fn(1) == 0
            assert fn(5) == 1  # nonzero = on
            assert fn(0) == 1
        finally:
            fn(prev)
        assert fn(prev) == prev


def test_phase_stats_read_resets():
    lib = _lib()
    out = (ctypes.c_ulonglong * 9)(*([7] * 9))
    assert lib.conflux_lu_debug_panel_phase_stats(out) == 0
    assert lib.conflux_lu_debug_panel_phase_stats(out) == 0
    assert list(out) == [0] * 9
    assert lib.conflux_lu_debug_panel_phase_stats(None) != 0
