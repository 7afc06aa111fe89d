"""-m "not gpu": the C-ABI shared library loads and exports every symbol include/emd_raster.h declares;
host-only entry points and argument validation work without a GPU (no compute calls here)."""
import ctypes as C
import os
import re
import subprocess

import pytest

from emd_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_functions():
    src = open(os.path.join(ROOT, "include", "emd_raster.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(emd_[a-z0-9_]+)\s*\(", src)))


def test_header_symbols_all_exported():
    lib = L.load()
    names = _declared_functions()
    assert len(names) >= 11
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/emd_raster.h but not exported"
    assert sorted(L.EXPORTED_SYMBOLS) == names


def test_abi_version_matches_header():
    src = open(os.path.join(ROOT, "include", "emd_raster.h")).read()
    v = int(re.search(r"#define EMD_ABI_VERSION (\d+)", src).group(1))
    assert L.load().emd_abi_version() == v == L.ABI_VERSION


# upper-case ints of _lib that the header does not name: the payload floats of an accumulator row and the pitch derived from them (csrc/common.h),
# and the floats of one camera-gradient row (csrc/camera_grad.hip)
CONSTANTS_WITHOUT_HEADER_NAME = {"BWD_PAYLOAD", "BWD_STRIDE", "CAMERA_GRAD_FLOATS"}


def _mirrored_constants():
    """{name of an upper-case int of _lib: the header names it must equal}; a name neither matched nor listed above maps to nothing and fails."""
    header = set(re.findall(r"\bEMD_[A-Z0-9_]+\b", open(os.path.join(ROOT, "include", "emd_raster.h")).read()))
    want = {}
    for name, v in vars(L).items():
        if not name.isupper() or isinstance(v, bool) or not isinstance(v, int) or name in CONSTANTS_WITHOUT_HEADER_NAME:
            continue
        c_name = name if name.startswith("EMD_") else "EMD_" + name
        want[name] = ["EMD_TILE_X", "EMD_TILE_Y"] if name == "TILE" else [c_name] if c_name in header else []
    return want


def test_struct_layout_matches_c(tmp_path):
    """The whole mirror against the C compiler in one program: sizeof of every ctypes.Structure of _lib, offsetof and sizeof of every field its
    `_fields_` names (a name the header does not have fails the compile), and every integer constant of _lib the header names."""
    structs = [t for t in vars(L).values() if isinstance(t, type) and issubclass(t, C.Structure) and t.__module__ == L.__name__]
    constants = _mirrored_constants()
    assert len(structs) >= 40 and all(constants.values()), [n for n, c in constants.items() if not c]
    acts = {f"EMD_NSTD_ACT_{k.upper()}": v for k, v in L.NSTD_ACT.items()}
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "emd_raster.h"', 'int main(void){', 'printf("S EmdStatus - %zu 0\\n", sizeof(EmdStatus));']
    for t in structs:
        n = t.__name__
        lines.append(f'printf("S {n} - %zu 0\\n", sizeof({n}));')
        lines += [f'printf("F {n} {f} %zu %zu\\n", offsetof({n}, {f}), sizeof((({n} *)0)->{f}));' for f, *_ in t._fields_]
    lines += [f'printf("K {c} - %lld 0\\n", (long long)({c}));' for c in sorted({c for cs in constants.values() for c in cs} | set(acts))]
    lines.append("return 0;}")
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = {(kind, a, b): (int(x), int(y)) for kind, a, b, x, y in (ln.split() for ln in subprocess.check_output([str(exe)], text=True).splitlines())}
    want = {("S", "EmdStatus", "-"): (16, 0)}
    for t in structs:
        want["S", t.__name__, "-"] = (C.sizeof(t), 0)
        want.update({("F", t.__name__, f): (getattr(t, f).offset, getattr(t, f).size) for f, *_ in t._fields_})
    want.update({("K", c, "-"): (getattr(L, name), 0) for name, cs in constants.items() for c in cs})
    want.update({("K", c, "-"): (v, 0) for c, v in acts.items()})
    assert got.keys() == want.keys()
    wrong = [f"{' '.join(k)}: C (offset or value, size) {got[k]}, ctypes {want[k]}" for k in want if got[k] != want[k]]
    assert not wrong, "\n".join(wrong)


def test_workspace_size_host_only():
    g, b, i, w = L.workspace_sizes(2_000_000, 1066, 1600, 8_000_000)
    assert g >= 2_000_000 * 64 and b >= 8_000_000 * 16 and i >= 1066 * 1600 * 8 and w == 2_000_000 * L.BWD_STRIDE * 4
    # grows monotonically with capacity, zero Gaussians allowed
    assert L.workspace_sizes(0, 16, 16, 0)[0] > 0
    assert L.workspace_sizes(10, 64, 64, 1000)[1] < L.workspace_sizes(10, 64, 64, 100000)[1]


def test_invalid_arguments_report_errors():
    lib = L.load()
    d = L.EmdDims(-1, 10, 10, 0, 0)
    out = (C.c_size_t * 4)()
    assert lib.emd_raster_workspace_size(C.byref(d), out) == L.EMD_ERR_INVALID
    assert b"bad dims" in lib.emd_last_error()
    a = L.EmdFwdArgs()
    a.num_gaussians = 5
    a.s.image_height = a.s.image_width = 32
    # neither means nor opacities -> invalid, reported before any HIP call
    assert lib.emd_raster_forward(C.byref(a), None) == L.EMD_ERR_INVALID
    assert b"null" in lib.emd_last_error()
    with pytest.raises(L.EmdError):
        L.check(L.EMD_ERR_INVALID, "x")


def test_rasterizer_rejects_cpu_tensors_and_bad_combinations():
    import torch
    from emd_amd import GaussianRasterizationSettings, GaussianRasterizer
    rs = GaussianRasterizationSettings(16, 16, 1.0, 1.0, torch.zeros(3), 1.0, torch.eye(4), torch.eye(4), 0,
                                       torch.zeros(3), False, False)
    r = GaussianRasterizer(rs)
    m = torch.zeros(4, 3)
    with pytest.raises(Exception, match="excatly one"):
        r(means3D=m, means2D=m, opacities=torch.ones(4, 1), shs=None, colors_precomp=None, scales=m, rotations=torch.ones(4, 4))
    with pytest.raises(Exception, match="exactly one"):
        r(means3D=m, means2D=m, opacities=torch.ones(4, 1), colors_precomp=m, scales=m, rotations=None)
    with pytest.raises(NotImplementedError):
        r(means3D=m, means2D=m, opacities=torch.ones(4, 1), colors_precomp=m, scales=m, rotations=torch.ones(4, 4), extra_attrs=m)
    # no CPU fallback: CPU tensors must fail loudly
    with pytest.raises(L.EmdError, match="no CPU path"):
        r(means3D=m, means2D=m, opacities=torch.ones(4, 1), colors_precomp=m, scales=m, rotations=torch.ones(4, 4))
