"""The plumbing the six libraries share, without a GPU and without a built library: _dl.open_library answers a missing file, a library
without a version symbol, one of another version and one that lacks an export with the ImportError the binding modules have always
raised, and declares every signature on success; build.LIBRARIES is the one table behind build.py's public names."""
import ctypes
import os

import pytest

from pykrige_amd import _dl, build

SIGNATURES = {
    "abc_abi_version": (ctypes.c_int, []),
    "abc_last_error": (ctypes.c_char_p, []),
    "abc_work": (ctypes.c_int, [ctypes.c_int64, ctypes.POINTER(ctypes.c_double)]),
}


class Fake:
    """A stand-in for what ctypes.CDLL returns: the named functions, the version one answering ``version``."""

    def __init__(self, version, names):
        for name in names:
            fn = (lambda: version) if name == "abc_abi_version" else (lambda *a: 0)
            setattr(self, name, fn)


def test_open_library_answers_a_missing_or_stale_library_and_declares_the_signatures(monkeypatch, tmp_path):
    with pytest.raises(ImportError, match=r"no_such_library.so is missing -- build it with `python -m pykrige_amd.build` \(needs hipcc; "
                                          r"there is no CPU fallback\)"):
        _dl.open_library(str(tmp_path / "no_such_library.so"), "abc", 3, SIGNATURES)
    path = tmp_path / "libabc.so"
    path.write_bytes(b"")
    opened = []

    def cdll(fake):
        def open_(p):
            opened.append(p)
            return fake
        return open_

    # reached through ctypes at call time: the host tests of the libraries replace ctypes.CDLL
    monkeypatch.setattr(ctypes, "CDLL", cdll(Fake(3, [])))
    with pytest.raises(ImportError, match=r"libabc.so has no abc_abi_version, this package was written against ABI version 3 -- rebuild it "
                                          r"\(`python -m pykrige_amd.build --force`\)"):
        _dl.open_library(str(path), "abc", 3, SIGNATURES)
    assert opened == [str(path)]
    monkeypatch.setattr(ctypes, "CDLL", cdll(Fake(2, list(SIGNATURES))))
    with pytest.raises(ImportError, match=r"libabc.so has ABI version 2, this package was written against ABI version 3 -- rebuild it"):
        _dl.open_library(str(path), "abc", 3, SIGNATURES)
    # the version is asked first: a library that lacks an export and has the wrong version is answered with the version
    monkeypatch.setattr(ctypes, "CDLL", cdll(Fake(2, ["abc_abi_version"])))
    with pytest.raises(ImportError, match="has ABI version 2"):
        _dl.open_library(str(path), "abc", 3, SIGNATURES)
    monkeypatch.setattr(ctypes, "CDLL", cdll(Fake(3, ["abc_abi_version", "abc_last_error"])))
    with pytest.raises(ImportError, match=r"libabc.so does not export abc_work, this package was written against ABI version 3 -- rebuild it") as e:
        _dl.open_library(str(path), "abc", 3, SIGNATURES)
    assert e.value.__suppress_context__  # no bare AttributeError behind it
    fake = Fake(3, list(SIGNATURES))
    monkeypatch.setattr(ctypes, "CDLL", cdll(fake))
    assert _dl.open_library(str(path), "abc", 3, SIGNATURES) is fake
    for name, (res, args) in SIGNATURES.items():
        assert getattr(fake, name).restype is res and getattr(fake, name).argtypes == args, name


def test_raise_for_and_device(monkeypatch):
    class Lib:
        abc_last_error = staticmethod(lambda: b"the reason")

    with pytest.raises(ValueError, match="^the reason$"):
        _dl.raise_for(Lib, "abc", "libabc", -1, -1)
    with pytest.raises(RuntimeError, match=r"^libabc: the reason \(code -3\)$"):
        _dl.raise_for(Lib, "abc", "libabc", -3, -1)
    Lib.abc_last_error = staticmethod(lambda: None)
    with pytest.raises(RuntimeError, match=r"^libabc:  \(code -3\)$"):
        _dl.raise_for(Lib, "abc", "libabc", -3, -1)
    monkeypatch.delenv("MIK_DEVICE", raising=False)
    monkeypatch.delenv("LOCAL_RANK", raising=False)
    assert _dl.device() == 0
    monkeypatch.setenv("LOCAL_RANK", "3")
    assert _dl.device() == 3
    monkeypatch.setenv("MIK_DEVICE", "5")
    assert _dl.device() == 5


def test_the_binding_modules_load_through_open_library(monkeypatch):
    from pykrige_amd import _lib, likelihood, variography, variography3d, vecchia

    calls = []
    monkeypatch.setattr(_dl, "open_library", lambda *a: calls.append(a) or "the library")
    for mod, load, cache, prefix, path, version, table in (
            (_lib, "load", "_lib", "mik", "LIB_PATH", "ABI_VERSION", "SIGNATURES"),
            (variography, "load", "_lib", "mkv", "LIB_PATH", "ABI_VERSION", "SIGNATURES"),
            (variography3d, "load", "_lib", "mkv3", "LIB_PATH", "ABI_VERSION", "SIGNATURES"),
            (likelihood, "load", "_lib", "mlk", "LIB_PATH", "ABI_VERSION", "SIGNATURES"),
            (likelihood, "load_grad", "_lib_grad", "mlg", "LIB_PATH_GRAD", "ABI_VERSION_GRAD", "SIGNATURES_GRAD"),
            (vecchia, "load", "_lib", "mvc", "LIB_PATH", "ABI_VERSION", "SIGNATURES")):
        monkeypatch.setattr(mod, cache, None)
        monkeypatch.setattr(mod, path, "/somewhere/else.so")  # read at call time
        assert getattr(mod, load)() == "the library" and getattr(mod, cache) == "the library"
        assert calls[-1] == ("/somewhere/else.so", prefix, getattr(mod, version), getattr(mod, table))
        assert all(name.startswith(prefix + "_") for name in getattr(mod, table)) and prefix + "_abi_version" in getattr(mod, table)
        n = len(calls)
        assert getattr(mod, load)() == "the library" and len(calls) == n  # cached


def test_the_libraries_table_is_behind_every_public_name_of_the_build():
    libs = build.LIBRARIES
    assert len(libs) == 6
    assert [os.path.basename(lib.out) for lib in libs] == ["libmikrige.so", "libmikvario.so", "libmikvario3.so", "libmiklik.so",
                                                           "libmikgrad.so", "libmikvecchia.so"]
    assert all(os.path.basename(lib.out) in build.__doc__ for lib in libs)
    assert [build.OUT, build.OUT_VARIO, build.OUT_VARIO3, build.OUT_LIK, build.OUT_GRAD, build.OUT_VECCHIA] == [lib.out for lib in libs]
    assert [build.API, build.API_VARIO, build.API_VARIO3, build.API_LIK, build.API_GRAD, build.API_VECCHIA] == [lib.api for lib in libs]
    units = [build.UNITS, build.UNITS_VARIO, build.UNITS_VARIO3, build.UNITS_LIK, build.UNITS_GRAD, build.UNITS_VECCHIA]
    assert all(lib.units is u for lib, u in zip(libs, units))
    assert [len(u) for u in units] == [10, 1, 1, 1, 1, 1] and len({n for u in units for n in u}) == 15  # one object file each
    assert [os.path.basename(lib.api) for lib in libs] == ["mikrige.h", "mikvario.h", "mikvario3.h", "miklik.h", "mikgrad.h", "mikvecchia.h"]
    assert all(os.path.dirname(lib.api) == os.path.join(build.ROOT, "include") and os.path.exists(lib.api) for lib in libs)
    assert libs[0].common == build.COMMON == ["mik_host.h", "mik_dev.h"] and all(lib.common == [] for lib in libs[1:])
    assert libs[0].tail == ["-ldl", "-Wl,-s"] and all(lib.tail == ["-Wl,-s"] for lib in libs[1:])
    deps = [build.unit_deps, build.vario_deps, build.vario3_deps, build.lik_deps, build.grad_deps, build.vecchia_deps]
    for lib, of in zip(libs, deps):
        for name, unit in lib.units.items():
            want = [os.path.join(build.CSRC, f) for f in [unit[0]] + unit[1] + lib.common] + [lib.api]
            assert of(name) == lib.deps(name) == want, name
            assert all(os.path.exists(d) for d in want), name
    assert build.all_sources() == libs[0].sources() and len(build.all_sources()) == len(set(build.all_sources()))
    assert set(build.all_sources()) == {d for name in build.UNITS for d in build.unit_deps(name)}
    assert all(lib.sources() == lib.deps(next(iter(lib.units))) for lib in libs[1:])


def test_a_tree_built_under_another_path_is_not_up_to_date(monkeypatch):
    """The command line of every object is kept beside it; a checkout that was moved or copied after its build records another include
    path, and ``up_to_date`` must say so, so that ``build_library`` recompiles instead of handing out objects of another command line.
    The compression flags are no difference (a hipcc without them records their absence), nor is an object without a stamp."""
    build.build_library()
    assert build.up_to_date()
    moved = [c if not c.startswith("-I") else "-I" + os.path.join(os.sep, "elsewhere", "include") for c in build.FLAGS]
    monkeypatch.setattr(build, "FLAGS", moved)
    assert not build.up_to_date()
    monkeypatch.undo()
    assert build.up_to_date()
    monkeypatch.setattr(build, "FLAGS", [c for c in build.FLAGS if c not in build.COMPRESS])
    assert build.up_to_date()
    monkeypatch.undo()
    monkeypatch.setattr(build, "OBJ", os.path.join(build.OBJ, "no_such_directory"))
    assert build.up_to_date()
