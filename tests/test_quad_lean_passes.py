"""
Three generator switches of the single-mode quad kernels (``csrc/okx_quadgen.cpp``; ``tools/README.md``), each of which
restores the earlier text of one piece of quad-uniform scalar work taken out of the Levenberg-Marquardt passes:

  quad_atan_branches   lean_atan2_pos as an if / else chain over its five ranges (default: selected constants, no branch)
  quad_column_pivots   the cold fast loop's pivot statistics on every column's broadcast pivot (default: per lane, one
                       reduction per pass)
  quad_fmax_calls      fmax / fmin calls (default: bare v_max_f64 / v_min_f64 where the operand would be quieted first)

The double-wishbone module's text is deterministic under every setting (the text is the kernel cache key), each switch
changes what it names and nothing else, and every text compiles with hiprtc for gfx950 - no device needed (after build()
these are cache hits; in a fresh cache each is a real compilation).  CPU only.
"""

import ctypes as C

import pytest

from open_kinematics_amd import _abi, _lib

SWITCHES = ["quad_atan_branches", "quad_column_pivots", "quad_fmax_calls"]


def _corner():
    from open_kinematics_amd.workloads import bump_sweep_problem

    return bump_sweep_problem(4)[0]


def _source(program) -> str:
    lib = _lib.load()
    host = _abi.HostProgram(program)  # (keeps views of the program's arrays: the caller holds the program)
    size = lib.okx_quad_source(host.byref(), None, 0)
    if size < 0:
        raise ValueError(_lib.last_error())
    buf = C.create_string_buffer(size)
    assert lib.okx_quad_source(host.byref(), buf, size) == size
    return buf.value.decode()


def _texts(monkeypatch, program):
    texts = {}
    for setting in [""] + SWITCHES + [",".join(SWITCHES)]:
        if setting:
            monkeypatch.setenv("OKX_DEV", setting)
        else:
            monkeypatch.delenv("OKX_DEV", raising=False)
        first, second = _source(program), _source(program)
        assert first == second, f"OKX_DEV={setting!r}: the same setting must give the same text every time"
        texts[setting] = first
    monkeypatch.delenv("OKX_DEV", raising=False)
    return texts


def test_each_switch_changes_its_own_text_only(monkeypatch):
    texts = _texts(monkeypatch, _corner())
    default, old = texts[""], texts[",".join(SWITCHES)]
    assert len(set(texts.values())) == len(texts)
    # the default text: one reciprocal sequence after t's own and no range branch in lean_atan2_pos, the per-lane pivot
    # range in the fast loop only, the bare maxima and the helpers they call
    atan = default[default.index("DEV double lean_atan2_pos("):default.index("DEV bool wave_any(")]
    assert atan.count("fast_rcp(") == 2 and "else if" not in atan and "return x >= 0.0" not in atan
    assert default.count("pmin = PMIN(") == 1 and default.count("pmin = fmin(pmin, piv)") >= 1
    assert "bare_max_abs(mres_new" in default and default.count("DEV double bare_max_abs(") == 1
    # the earlier text knows none of it
    for word in ("PMIN", "bare_m", "qmin", "qmax_bare"):
        assert word not in old, word
    atan_old = old[old.index("DEV double lean_atan2_pos("):old.index("DEV bool wave_any(")]
    assert atan_old.count("fast_rcp(") == 5 and atan_old.count("else if") == 3
    # one switch, one difference
    assert "else if (t < 0.6875)" in texts["quad_atan_branches"] and "PMIN(" in texts["quad_atan_branches"]
    assert "PMIN" not in texts["quad_column_pivots"] and "bare_max_abs(mres_new" in texts["quad_column_pivots"]
    assert "bare_m" not in texts["quad_fmax_calls"] and "pmin = PMIN(" in texts["quad_fmax_calls"] and "DEV double qmin(" in texts["quad_fmax_calls"]


@pytest.mark.parametrize("setting", [""] + SWITCHES)
def test_the_corner_module_compiles_without_a_device(monkeypatch, setting):
    if setting:
        monkeypatch.setenv("OKX_DEV", setting + ",no_lane")
    else:
        monkeypatch.setenv("OKX_DEV", "no_lane")  # (the lane module's text does not change with these switches)
    program = _corner()
    host = _abi.HostProgram(program)
    rc = _lib.load().okx_precompile(host.byref())
    assert rc == 0, _lib.last_error()
