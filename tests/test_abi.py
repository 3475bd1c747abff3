"""CPU: the C-ABI library loads and exports every symbol include/tissue_hip.h declares, with the argument types
_abi.SIGNATURES gives them (no device calls)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    text = open(os.path.join(ROOT, "include", "tissue_hip.h")).read()
    return sorted(set(re.findall(r"TIP_API\s+int\s+(tip_\w+)\s*\(", text)))


def declared_signatures():
    """{name: (return type, argtypes)} of every TIP_API prototype, in the header's order; a prototype that does not parse
    raises."""
    from tissue_image_processing_amd import _abi
    scalars = {"int": _abi.I, "int32_t": _abi.I, "int64_t": _abi.L, "long": _abi.L, "size_t": _abi.Z, "double": _abi.D,
               "float": _abi.F}
    text = open(os.path.join(ROOT, "include", "tissue_hip.h")).read()
    text = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    text = re.sub(r"#define\s+TIP_API\b[^\n]*", "", text)
    protos = re.findall(r"TIP_API\s+(\w+)\s+(tip_\w+)\s*\(([^()]*)\)\s*;", text)
    assert len(protos) == len(re.findall(r"\bTIP_API\b", text)), "a TIP_API prototype did not parse"
    out = {}
    for ret, name, params in protos:
        sig = []
        for p in ([] if params.strip() == "void" else params.split(",")):
            if "*" in p:
                sig.append(_abi.P)
            else:
                ctype, _pname = [t for t in p.split() if t != "const"]
                sig.append(scalars[ctype])
        assert name not in out, name
        out[name] = (ret, tuple(sig))
    return out


def test_signature_table_is_the_header():
    """_abi.SIGNATURES against include/tissue_hip.h: the same names in the same order, every argument type equal under the six
    mapping rules, every return type int (what _lib.load() declares)."""
    from tissue_image_processing_amd import _abi
    header = declared_signatures()
    assert sorted(header) == declared_symbols()
    assert list(_abi.SIGNATURES) == list(header)
    for name, (ret, sig) in header.items():
        assert ret == "int", name
        assert _abi.SIGNATURES[name] == sig, name


def test_declared_entry_takes_plain_numbers():
    """tip_gaussian_taps touches no device: plain Python and numpy numbers arrive as the header's double and int."""
    import numpy as np
    from tissue_image_processing_amd import _lib
    lib = _lib.load()
    w = np.zeros(64)
    assert lib.tip_gaussian_taps(1.0, 4.0, _lib.ptr(w), 64) == 9
    assert w[:9].sum() == 1.0
    assert lib.tip_gaussian_taps(np.float32(1.0), 4, _lib.ptr(w), np.int64(64)) == 9


def test_declared_entry_rejects_mistakes():
    import numpy as np
    from tissue_image_processing_amd import _lib
    lib = _lib.load()
    w = np.zeros(64)
    with pytest.raises(TypeError):
        lib.tip_gaussian_taps(1.0, 4.0, _lib.ptr(w))
    with pytest.raises(ctypes.ArgumentError):
        lib.tip_gaussian_taps(1.0, 4.0, _lib.ptr(w), 2.5)


def test_header_declares_the_hot_path():
    syms = declared_symbols()
    for s in ["tip_init", "tip_last_error", "tip_shutdown", "tip_gaussian3d_f32", "tip_project_u16", "tip_rankfilter2d",
              "tip_label4_i32", "tip_watershed_f64", "tip_regionprops_i32", "tip_neighbor_pairs_i32"]:
        assert s in syms


def test_library_exports_every_declared_symbol():
    from tissue_image_processing_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    missing = [s for s in declared_symbols() if not hasattr(lib, s)]
    assert not missing, "symbols declared in include/tissue_hip.h but not exported: %s" % missing
    assert lib.tip_version() >= 100


def test_product_fails_loudly_without_gpu():
    """No CPU fallback: on a box without a HIP device every operator raises (the product never imports oracle/)."""
    import numpy as np
    from tissue_image_processing_amd import _lib
    lib = _lib.load()
    if lib.tip_device_count() > 0:
        pytest.skip("GPU present")
    from tissue_image_processing_amd import basic_image_manipulations as bim
    with pytest.raises(_lib.TissueHipError):
        bim.blur_image(np.zeros((4, 4), np.float32), 1.0)


def test_product_never_imports_oracle():
    pkg = os.path.join(ROOT, "tissue_image_processing_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h")):
                text = open(os.path.join(dirpath, f)).read()
                assert "import oracle" not in text and "from oracle" not in text, f
                assert "tip_oracle" not in text, f


def test_host_axis_logic():
    import numpy as np
    from tissue_image_processing_amd.basic_image_manipulations import put_channel_axis_first
    a = np.zeros((3, 2, 5, 7))          # Z C Y X
    out, order = put_channel_axis_first(a, "ZCYX")
    assert out.shape == (2, 3, 7, 5) and order == (1, 0, 3, 2)     # reference order is C,(Z),X,Y (bim.py:219-226)
    out, order = put_channel_axis_first(a, "CZYX")                 # C already first: untouched (bim.py:216 `> 0`)
    assert out is a and tuple(order) == (0, 1, 2, 3)


PROJECTION_HOOKS = ("TIP_PROJECT_EXACT_SCORE", "TIP_PROJECT_GENERIC", "TIP_PROJECT_UNFUSED_PREBLUR", "TIP_PROJECT_UNFUSED_MASK",
                    "TIP_PROJECT_DEBUG")


def test_retired_score_pass_hooks_are_unknown():
    """The float32 / VALU score-pass flavours are gone, and with them their hooks (tip_set_tuning touches no device)."""
    from tissue_image_processing_amd import _lib
    with pytest.raises(ValueError):
        _lib.set_tuning("TIP_FAST_CFG", "5,5")
    with pytest.raises(ValueError):
        _lib.set_tuning("TIP_MFMA_BLOCKS_PER_CU", "1")


@pytest.mark.parametrize("name", PROJECTION_HOOKS)
def test_projection_hooks_are_accepted(name):
    from tissue_image_processing_amd import _lib
    try:
        _lib.set_tuning(name, "1")
    finally:
        _lib.set_tuning(name, None)


def test_tests_switch_hooks_through_the_library():
    """The library reads the TIP_* environment once per process: a hook set in the environment after the first call never
    reaches it, and the test would compare the default path with itself.  Tests switch hooks with _lib.tuning."""
    pat = re.compile(r"""(setenv|setdefault)\(\s*["']TIP_|os\.environ\[\s*["']TIP_\w*["']\s*\]\s*=(?!=)""")
    tests = os.path.join(ROOT, "tests")
    hits = []
    for f in sorted(os.listdir(tests)):
        if f.endswith(".py"):
            with open(os.path.join(tests, f)) as fh:
                hits += ["%s:%d: %s" % (f, i, line.strip()) for i, line in enumerate(fh, 1) if pat.search(line)]
    assert not hits, "hooks switched through the environment:\n" + "\n".join(hits)
