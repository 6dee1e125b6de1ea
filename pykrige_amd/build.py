"""Builds pykrige_amd/libmikrige.so, pykrige_amd/libmikvario.so, pykrige_amd/libmikvario3.so, pykrige_amd/libmiklik.so, pykrige_amd/libmikgrad.so and pykrige_amd/libmikvecchia.so (HIP, gfx950) in-tree.  `python -m pykrige_amd.build [--force] [-j N]`.

The library is ten translation units compiled in parallel (objects under pykrige_amd/csrc/build/, git- and gpurun-ignored) and
linked into one shared object; only the units whose sources or flags changed are recompiled (the command line of every object is
kept beside it as <name>.flags).  Safe against concurrent callers (pytest-xdist, one process per GPU calling __graft_entry__.build):
the whole build holds an flock on csrc/build/.lock, and objects / the library are written under a per-process name and renamed into place.

    mikrige.hip       C ABI, handles, device groups + factor exchange, K1 assembly, points / grids / masks, statistics
    mik_inverse.hip   K2: block Gauss-Jordan sweep and its schedules, probes, pseudo-inverses
    mik_predict.hip   K3: right-hand sides, dense and range-aware contraction, point sort
    mik_mw.hip        moving window: neighbour search, blocked / HBM solvers, dispatch
    mik_mw_solve.hip  moving window: the register classes of the pivoting Gauss-Jordan solver (the LDL^T kernels' fallback)
    mik_mw_chol.hip   x 5 (-DMIK_MWC_PART=0..4): the register-tile classes of the moving window's LDL^T solver

Five further libraries of one unit each are built after the first with the same flags under the same lock and rename discipline:
libmikvario.so (mik_vario.hip, include/mikvario.h: directional semivariograms and variogram maps), libmikvario3.so (mik_vario3.hip,
include/mikvario3.h: the same tools for the 3-D classes), libmiklik.so (mik_lik.hip, include/miklik.h: log det C and W^T C^-1 W for the
ML / REML fit of likelihood.py), libmikgrad.so (mik_grad.hip, include/mikgrad.h: the same two numbers and the analytic gradient; its unit
includes mik_k_lik.h, unchanged, and compiles the four elimination kernels into itself) and libmikvecchia.so (mik_vecchia.hip,
include/mikvecchia.h: the same two numbers under Vecchia's approximation, for vecchia.py).  They exist because libmikrige.so is held to a
size bar and a frozen kernel list (tests/test_abi_and_host.py), and each later library's exports and kernels are pinned by its own host
test: new device features get a shared object of their own.  Each unit includes its own headers only, and no object is linked between
the six.

LIBRARIES is the one table of all this: a library is one record of it, and a binding module that calls _dl.open_library.

EXTRA_LIBRARIES holds the records after the sixth -- libmikvgrad.so (mik_vgrad.hip, include/mikvgrad.h: Vecchia's two numbers and their
analytic derivatives, for vecchia_grad.py; its unit includes mik_k_vecchia.h, unchanged, and compiles the three k_vec_* kernels into
itself beside its own mik_k_vgrad.h).  The second list exists only because the table test pins the first at six records; every loop of
the build runs over LIBRARIES + EXTRA_LIBRARIES.
"""
import os
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(HERE, "csrc")
OBJ = os.path.join(CSRC, "build")
COMMON = ["mik_host.h", "mik_dev.h"]
# object name -> (source, extra headers it includes, extra flags)
UNITS = {
    "mikrige": ("mikrige.hip", ["mik_k_core.h"], []),
    "mik_inverse": ("mik_inverse.hip", ["mik_k_inverse.h"], []),
    "mik_predict": ("mik_predict.hip", ["mik_k_predict.h", "mik_k_fields.h", "mik_k_cvfolds.h", "mik_k_gaps.h", "mik_k_cov.h", "mik_k_block.h"], []),
    "mik_mw": ("mik_mw.hip", ["mik_k_mw.h", "mik_k_mw_chol.h"], []),
    "mik_mw_solve": ("mik_mw_solve.hip", ["mik_k_mw_solve.h", "mik_k_mw_chol.h"], []),
    "mik_mw_chol0": ("mik_mw_chol.hip", ["mik_k_mw_chol.h"], ["-DMIK_MWC_PART=0"]),
    "mik_mw_chol1": ("mik_mw_chol.hip", ["mik_k_mw_chol.h"], ["-DMIK_MWC_PART=1"]),
    "mik_mw_chol2": ("mik_mw_chol.hip", ["mik_k_mw_chol.h"], ["-DMIK_MWC_PART=2"]),
    "mik_mw_chol3": ("mik_mw_chol.hip", ["mik_k_mw_chol.h"], ["-DMIK_MWC_PART=3"]),
    "mik_mw_chol4": ("mik_mw_chol.hip", ["mik_k_mw_chol.h"], ["-DMIK_MWC_PART=4"]),
}
# the later libraries: object name -> (source, headers it includes); their own headers only, so a change of the first library's leaves them
# alone.  (The fifth runs the fourth's elimination kernels, so their header is a dependency.)
UNITS_VARIO = {"mik_vario": ("mik_vario.hip", ["mik_k_vario.h"])}
UNITS_VARIO3 = {"mik_vario3": ("mik_vario3.hip", ["mik_k_vario3.h"])}
UNITS_LIK = {"mik_lik": ("mik_lik.hip", ["mik_k_lik.h"])}
UNITS_GRAD = {"mik_grad": ("mik_grad.hip", ["mik_k_grad.h", "mik_k_lik.h"])}
UNITS_VECCHIA = {"mik_vecchia": ("mik_vecchia.hip", ["mik_k_vecchia.h"])}
UNITS_VGRAD = {"mik_vgrad": ("mik_vgrad.hip", ["mik_k_vgrad.h", "mik_k_vecchia.h"])}


class Library:
    """One shared object: its path, its API header, its units, the headers every unit includes and the end of its link line."""

    def __init__(self, name, header, units, common=(), tail=("-Wl,-s",)):
        self.out = os.path.join(HERE, name)
        self.api = os.path.join(ROOT, "include", header)
        self.units, self.common, self.tail = units, list(common), list(tail)

    def deps(self, name):
        src, hdrs = self.units[name][:2]
        return [os.path.join(CSRC, f) for f in [src] + hdrs + self.common] + [self.api]

    def sources(self):
        seen = []
        for name in self.units:
            for d in self.deps(name):
                if d not in seen:
                    seen.append(d)
        return seen


# (-s: no static symbol table -- 90 kB; the C ABI and the kernels' host stubs are dynamic symbols, `nm -D` lists them)
LIBRARIES = [
    Library("libmikrige.so", "mikrige.h", UNITS, COMMON, ["-ldl", "-Wl,-s"]),
    Library("libmikvario.so", "mikvario.h", UNITS_VARIO),
    Library("libmikvario3.so", "mikvario3.h", UNITS_VARIO3),
    Library("libmiklik.so", "miklik.h", UNITS_LIK),
    Library("libmikgrad.so", "mikgrad.h", UNITS_GRAD),
    Library("libmikvecchia.so", "mikvecchia.h", UNITS_VECCHIA),
]
OUT, OUT_VARIO, OUT_VARIO3, OUT_LIK, OUT_GRAD, OUT_VECCHIA = (lib.out for lib in LIBRARIES)
API, API_VARIO, API_VARIO3, API_LIK, API_GRAD, API_VECCHIA = (lib.api for lib in LIBRARIES)
unit_deps, vario_deps, vario3_deps, lik_deps, grad_deps, vecchia_deps = (lib.deps for lib in LIBRARIES)
all_sources = LIBRARIES[0].sources
# the libraries after the sixth: built, checked and linked with the six (to be merged into LIBRARIES when its table test is next revised)
EXTRA_LIBRARIES = [Library("libmikvgrad.so", "mikvgrad.h", UNITS_VGRAD)]
OUT_VGRAD, API_VGRAD, vgrad_deps = EXTRA_LIBRARIES[0].out, EXTRA_LIBRARIES[0].api, EXTRA_LIBRARIES[0].deps
# --offload-compress: the code objects travel zstd-compressed inside the fat binary (16.9 -> 2.3 MB of .so; the HIP runtime unpacks them at load);
# level 19 instead of the default 3 takes another 3 % off and no measurable compile time (the time is in code generation)
COMPRESS = ["--offload-compress", "--offload-compression-level=19"]
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC"] + COMPRESS + ["-I" + os.path.join(ROOT, "include")]
# seconds of one core per unit (hipcc of ROCm 7.2): the order the units are started in, longest first
COST = {"mik_vgrad": 60, "mik_mw_chol": 23, "mik_mw_solve": 15, "mik_predict": 12, "mikrige": 9, "mik_inverse": 6, "mik_mw": 4}


def hipcc():
    for c in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if c and os.path.exists(c):
            return c
    raise RuntimeError("hipcc not found (need ROCm; set HIPCC=/path/to/hipcc)")


def _stale(target, deps, flags=None):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    if any(os.path.getmtime(d) > t for d in deps):
        return True
    if flags is not None:  # built with another command line (e.g. the fallback without --offload-compress): stale
        try:
            return open(target[:-2] + ".flags").read() != " ".join(flags)
        except OSError:
            return True
    return False


def up_to_date():
    """Every library is newer than its sources, and no object's recorded command line differs from this checkout's -- a tree that was
    moved or copied after it was built records another include path.  (The compression flags aside: a hipcc without them records their
    absence.  An object without a stamp -- the build directory was not shipped -- is taken on its library's age.)"""
    plain = lambda flags: [c for c in flags if c not in COMPRESS]
    for lib in LIBRARIES + EXTRA_LIBRARIES:
        if _stale(lib.out, lib.sources()):
            return False
        for name, unit in lib.units.items():
            try:
                stamp = open(os.path.join(OBJ, name + ".flags")).read().split()
            except OSError:
                continue
            if plain(stamp) != plain(FLAGS + (unit[2] if len(unit) > 2 else [])):
                return False
    return True


def build_library(force=False, verbose=False, jobs=None):
    """Compile the seven C-ABI libraries for gfx950; returns the path of libmikrige.so (OUT; libmikvario.so is OUT_VARIO, libmikvario3.so
    OUT_VARIO3, libmiklik.so OUT_LIK, libmikgrad.so OUT_GRAD, libmikvecchia.so OUT_VECCHIA, libmikvgrad.so OUT_VGRAD).
    Cross-compiles without a GPU."""
    if not force and up_to_date():
        return OUT
    os.makedirs(OBJ, exist_ok=True)
    import fcntl

    with open(os.path.join(OBJ, ".lock"), "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)  # one builder at a time; the others find the work done when they get the lock
        if not force and up_to_date():
            return OUT
        return _build_locked(force, verbose, jobs)


def _build_locked(force, verbose, jobs):
    cc = hipcc()
    pid = ".%d.tmp" % os.getpid()
    todo, relink = [], []  # the compile jobs; the libraries to link
    for lib in LIBRARIES + EXTRA_LIBRARIES:
        before = len(todo)
        for name, unit in lib.units.items():
            obj = os.path.join(OBJ, name + ".o")
            flags = FLAGS + (unit[2] if len(unit) > 2 else [])
            if force or _stale(obj, lib.deps(name), flags):
                todo.append((name, flags, [cc] + flags + ["-c", os.path.join(CSRC, unit[0]), "-o", obj + pid]))
        if len(todo) > before or _stale(lib.out, lib.sources()):
            relink.append(lib)

    def run(job):
        name, flags, cmd = job
        if verbose:
            print(" ".join(cmd), flush=True)
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0 and COMPRESS[1] in cmd and "offload-compress" in r.stderr:
            # a hipcc that knows --offload-compress but not the level: the default level
            flags = [c for c in flags if c != COMPRESS[1]]
            cmd = [c for c in cmd if c != COMPRESS[1]]
            r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0 and COMPRESS[0] in cmd and "offload-compress" in r.stderr:
            # a hipcc that does not know the flag (before ROCm 6.1): the same objects, uncompressed -- and recorded as such, so that
            # a later build with a newer hipcc sees them as stale (the library is several times larger without the compression)
            flags = [c for c in flags if c not in COMPRESS]
            print("pykrige_amd.build: this hipcc does not know --offload-compress; %s is built uncompressed" % name, file=sys.stderr)
            r = subprocess.run([c for c in cmd if c not in COMPRESS], capture_output=True, text=True)
        obj = os.path.join(OBJ, name + ".o")
        if r.returncode != 0:
            if os.path.exists(obj + pid):
                os.remove(obj + pid)
            raise RuntimeError("compiling %s failed:\n%s" % (name, r.stderr[-4000:]))
        os.replace(obj + pid, obj)
        with open(obj[:-2] + ".flags", "w") as f:
            f.write(" ".join(flags))
        return name

    todo.sort(key=lambda j: -COST.get(j[0].rstrip("0123456789"), 0))  # (stable: the units without a cost keep the table's order, last)
    with ThreadPoolExecutor(max_workers=jobs or min(len(UNITS), os.cpu_count() or 4)) as ex:
        list(ex.map(run, todo))
    for lib in relink:
        objs = [os.path.join(OBJ, n + ".o") for n in lib.units]
        link = [cc, "--offload-arch=gfx950", "-shared", "-fPIC"] + objs + ["-o", lib.out + pid] + lib.tail
        if verbose:
            print(" ".join(link), flush=True)
        subprocess.run(link, check=True)
        os.replace(lib.out + pid, lib.out)
    return OUT


if __name__ == "__main__":
    j = int(sys.argv[sys.argv.index("-j") + 1]) if "-j" in sys.argv else None
    print(build_library(force="--force" in sys.argv, verbose=True, jobs=j))
