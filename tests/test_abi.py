"""CPU-side checks of the drop-in boundary: the C-ABI library builds, loads, and exports
every symbol ``include/happypose_amd.h`` declares (no compute calls -- no GPU here)."""

import ctypes
import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


def _declared_symbols():
    text = (ROOT / "include" / "happypose_amd.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(hp_[a-z0-9_]+)\s*\(", text)))


def test_header_symbols_exported():
    from happypose_amd import _ffi
    from happypose_amd.build import build

    build()
    lib = ctypes.CDLL(str(_ffi.lib_path()))
    declared = _declared_symbols()
    assert len(declared) >= 20
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in the header but not exported"
    # the Python binding covers exactly the header
    assert sorted(_ffi.EXPORTED_SYMBOLS) == declared


def test_op_kind_and_path_names_follow_the_header():
    """ops.OP_KINDS / ops.OP_PATHS name HP_OP_* / HP_PATH_* by value: same count, consecutive from 0, the last path is MIXED."""
    from happypose_amd import ops

    text = (ROOT / "include" / "happypose_amd.h").read_text()
    kinds = [int(v) for v in re.findall(r"#define HP_OP_[A-Z]+ (\d+)", text)]
    paths = re.findall(r"#define HP_PATH_([A-Z0-9_]+) (\d+)", text)
    assert kinds == list(range(len(ops.OP_KINDS)))
    assert [int(v) for _, v in paths] == list(range(len(ops.OP_PATHS)))
    assert paths[-1][0] == "MIXED" and ops.OP_PATHS[-1] == "mixed" and ops.OP_PATHS[0] == "none"
    for (name, _), mine in zip(paths, ops.OP_PATHS):
        assert mine.replace("+", "_").upper().replace("DW", "DWCONV") == name, (name, mine)


def test_no_cpu_fallback(monkeypatch, tmp_path):
    """The product path must fail loudly when the HIP library is missing."""
    from happypose_amd import _ffi

    monkeypatch.setattr(_ffi, "_lib", None)
    monkeypatch.setattr(_ffi, "_LIB_PATH", tmp_path / "nope.so")
    with pytest.raises(_ffi.HipLibraryError):
        _ffi.lib()


def test_product_does_not_import_oracle():
    """Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline may touch oracle/."""
    for py in (ROOT / "happypose_amd").rglob("*.py"):
        src = py.read_text()
        assert not re.search(r"^\s*(from|import)\s+oracle\b", src, flags=re.M), py


def test_argument_errors_reported_without_gpu():
    from happypose_amd import _ffi

    lib = _ffi.lib()
    assert lib.hp_version() >= 100
    rc = lib.hp_pose_update(-1, None, None, 9, None, None, None, None)
    assert rc == -1 and b"hp_pose_update" in lib.hp_last_error()
    with pytest.raises(AssertionError):
        _ffi.check(rc, "hp_pose_update")
    assert not lib.hp_net_create(7, 6, 240, 320)
    assert not lib.hp_mesh_store_create(None, None, None, None, 0, None, 0, None, 0, None, 0, None, 0)


def test_dynamic_symbols_are_the_header_only():
    """-fvisibility=hidden + csrc/exports.map: ``nm -D`` of the library shows the ``hp_*`` entry points of the header and nothing
    else (no ``hp::`` C++ helper, no kernel host stub)."""
    import subprocess

    from happypose_amd import _ffi

    out = subprocess.run(["nm", "-D", "--defined-only", str(_ffi.lib_path())], check=True, capture_output=True, text=True).stdout
    defined = sorted(line.split()[-1] for line in out.splitlines() if line.strip())
    assert defined == _declared_symbols(), sorted(set(defined) ^ set(_declared_symbols()))


def test_no_packed_fp32_arithmetic_in_the_device_code():
    """The build-time ISA check (happypose_amd/isa_check.py): no ``v_pk_fma/mul/add_f32`` in any gfx950 code
    object of the shipped library outside the exact-fp32 Winograd kernels' hand-placed ones -- and the checker does bite: the
    Winograd kernels, which do contain them, are found when the exception is lifted."""
    import re

    from happypose_amd import _ffi, isa_check

    assert isa_check.packed_f32_instructions(_ffi.lib_path()) == {}
    allowed, isa_check.ALLOWED_KERNELS = isa_check.ALLOWED_KERNELS, re.compile(r"$^")
    try:
        hits = isa_check.packed_f32_instructions(_ffi.lib_path())
    finally:
        isa_check.ALLOWED_KERNELS = allowed
    assert hits and all(allowed.search(k) for k in hits), sorted(hits)[:5]


def test_no_getenv_outside_the_debug_table():
    """One table of developer switches (csrc/debug.h / debug.cpp), read once, thread-safe; no ``getenv`` on any launch path."""
    for src in (ROOT / "happypose_amd" / "csrc").iterdir():
        if src.suffix in (".hip", ".cpp", ".h") and src.name != "debug.cpp":
            text = re.sub(r"//.*", "", src.read_text())
            assert "getenv" not in text, src.name
            assert not re.search(r"static\s+bool\s+(opted|done)", text), f"{src.name}: plain first-launch flag (use FirstLaunch)"


def test_first_launch_and_debug_table_are_race_free(tmp_path):
    """tests/host/first_launch_race.cpp under ThreadSanitizer: 16 host threads enter a kernel launcher's first-launch set-up
    (``hp::FirstLaunch``) and read the debug table for the first time at once -- one set-up, no data race report."""
    import os
    import shutil
    import subprocess

    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = tmp_path / "race"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=thread", "-D__HIP_PLATFORM_AMD__=1", "-I/opt/rocm/include",
           str(ROOT / "tests" / "host" / "first_launch_race.cpp"), str(ROOT / "happypose_amd" / "csrc" / "debug.cpp"), "-o", str(exe), "-pthread"]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    env = {**os.environ, "HP_PP_GRID": "64", "HP_NET_SYNC": "yes", "TSAN_OPTIONS": "halt_on_error=1 exitcode=66"}
    for k in ("HP_PROFILE_LAYERS", "HP_CONV_NO_PP"):
        env.pop(k, None)
    # GCC's TSan runtime expects the address layout of the default ASLR entropy: on kernels with more mmap randomisation bits it
    # aborts before main ("unexpected memory mapping").  The binary runs with address randomisation off for this one process
    # (personality ADDR_NO_RANDOMIZE) wherever setarch may set it.
    run = [str(exe)]
    arch = os.uname().machine
    if shutil.which("setarch") and subprocess.run(["setarch", arch, "-R", "true"], capture_output=True).returncode == 0:
        run = ["setarch", arch, "-R", str(exe)]
    r = subprocess.run(run, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout and "ThreadSanitizer" not in r.stderr, (r.returncode, r.stdout[-500:], r.stderr[-2000:])
