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

libmikvario.so (include/mikvario.h: directional semivariograms and variogram maps) is a second library of one unit, mik_vario.hip, built
after the first with the same flags under the same lock and rename discipline.  It exists because libmikrige.so is held to a size bar and
a frozen kernel list (tests/test_abi_and_host.py): new device features go here.  Nothing of it is linked into libmikrige.so or the reverse.

libmikvario3.so (include/mikvario3.h: the same tools for the 3-D classes -- directions by unit vector, maps of lag-vector cells in x, y, z)
is a third library of one unit, mik_vario3.hip, built the same way.  The second library's exports and kernels are pinned by
tests/test_directional_variogram_host.py, so the 3-D kernels have a shared object of their own; nothing is linked between the three.

libmiklik.so (include/miklik.h: log det C and W^T C^-1 W of a station set under a variogram model, for the ML / REML fit of likelihood.py)
is a fourth library of one unit, mik_lik.hip, built the same way: the second and third libraries are pinned by their host tests as the
first is, and the call needs no handle and no inverse.  Nothing is linked between the four.

libmikgrad.so (include/mikgrad.h: the same two numbers and the analytic gradient of the ML / REML objective, for the quasi-Newton fit of
likelihood.py) is a fifth library of one unit, mik_grad.hip, built the same way: the fourth library's exports and kernel list are pinned by
tests/test_likelihood_host.py.  Its unit includes mik_k_lik.h, unchanged, and compiles the four elimination kernels into itself; no object
is linked between the five.

libmikvecchia.so (include/mikvecchia.h: log det and W^T C^-1 W under Vecchia's approximation -- every station conditioned on at most m
earlier ones -- for the ML / REML fit of vecchia.py past the N x N matrix) is a sixth library of one unit, mik_vecchia.hip, built the same
way: the fourth and fifth libraries' exports and kernel lists are pinned by their host tests.  Its unit includes its own header only;
nothing is linked between the six.
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
OUT = os.path.join(HERE, "libmikrige.so")
OUT_VARIO = os.path.join(HERE, "libmikvario.so")
API = os.path.join(ROOT, "include", "mikrige.h")
API_VARIO = os.path.join(ROOT, "include", "mikvario.h")
OUT_VARIO3 = os.path.join(HERE, "libmikvario3.so")
API_VARIO3 = os.path.join(ROOT, "include", "mikvario3.h")
OUT_LIK = os.path.join(HERE, "libmiklik.so")
API_LIK = os.path.join(ROOT, "include", "miklik.h")
OUT_GRAD = os.path.join(HERE, "libmikgrad.so")
API_GRAD = os.path.join(ROOT, "include", "mikgrad.h")
OUT_VECCHIA = os.path.join(HERE, "libmikvecchia.so")
API_VECCHIA = os.path.join(ROOT, "include", "mikvecchia.h")
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
# the second library: object name -> (source, headers it includes); its own headers only, so a change of the first library's leaves it alone
UNITS_VARIO = {"mik_vario": ("mik_vario.hip", ["mik_k_vario.h"])}
# the third library, in the same form
UNITS_VARIO3 = {"mik_vario3": ("mik_vario3.hip", ["mik_k_vario3.h"])}
# the fourth library, in the same form
UNITS_LIK = {"mik_lik": ("mik_lik.hip", ["mik_k_lik.h"])}
# the fifth library, in the same form; it runs the fourth's elimination kernels, so their header is a dependency
UNITS_GRAD = {"mik_grad": ("mik_grad.hip", ["mik_k_grad.h", "mik_k_lik.h"])}
# the sixth library, in the same form
UNITS_VECCHIA = {"mik_vecchia": ("mik_vecchia.hip", ["mik_k_vecchia.h"])}
# --offload-compress: the code objects travel zstd-compressed inside the fat binary (16.9 -> 2.3 MB of .so; the HIP runtime unpacks them at load);
# level 19 instead of the default 3 takes another 3 % off and no measurable compile time (the time is in code generation)
COMPRESS = ["--offload-compress", "--offload-compression-level=19"]
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC"] + COMPRESS + ["-I" + os.path.join(ROOT, "include")]
# seconds of one core per unit (hipcc of ROCm 7.2): the order the units are started in, longest first
COST = {"mik_mw_chol": 23, "mik_mw_solve": 15, "mik_predict": 12, "mikrige": 9, "mik_inverse": 6, "mik_mw": 4}


def hipcc():
    for c in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if c and os.path.exists(c):
            return c
    raise RuntimeError("hipcc not found (need ROCm; set HIPCC=/path/to/hipcc)")


def unit_deps(name):
    src, hdrs, _ = UNITS[name]
    return [os.path.join(CSRC, f) for f in [src] + hdrs + COMMON] + [API]


def all_sources():
    seen = []
    for name in UNITS:
        for d in unit_deps(name):
            if d not in seen:
                seen.append(d)
    return seen


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


def vario_deps(name):
    src, hdrs = UNITS_VARIO[name]
    return [os.path.join(CSRC, f) for f in [src] + hdrs] + [API_VARIO]


def vario3_deps(name):
    src, hdrs = UNITS_VARIO3[name]
    return [os.path.join(CSRC, f) for f in [src] + hdrs] + [API_VARIO3]


def lik_deps(name):
    src, hdrs = UNITS_LIK[name]
    return [os.path.join(CSRC, f) for f in [src] + hdrs] + [API_LIK]


def grad_deps(name):
    src, hdrs = UNITS_GRAD[name]
    return [os.path.join(CSRC, f) for f in [src] + hdrs] + [API_GRAD]


def vecchia_deps(name):
    src, hdrs = UNITS_VECCHIA[name]
    return [os.path.join(CSRC, f) for f in [src] + hdrs] + [API_VECCHIA]


def up_to_date():
    return (not _stale(OUT, all_sources()) and not _stale(OUT_VARIO, [d for n in UNITS_VARIO for d in vario_deps(n)])
            and not _stale(OUT_VARIO3, [d for n in UNITS_VARIO3 for d in vario3_deps(n)])
            and not _stale(OUT_LIK, [d for n in UNITS_LIK for d in lik_deps(n)])
            and not _stale(OUT_GRAD, [d for n in UNITS_GRAD for d in grad_deps(n)])
            and not _stale(OUT_VECCHIA, [d for n in UNITS_VECCHIA for d in vecchia_deps(n)]))


def build_library(force=False, verbose=False, jobs=None):
    """Compile the six C-ABI libraries for gfx950; returns the path of libmikrige.so (OUT; libmikvario.so is OUT_VARIO, libmikvario3.so
    OUT_VARIO3, libmiklik.so OUT_LIK, libmikgrad.so OUT_GRAD, libmikvecchia.so OUT_VECCHIA).
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
    todo = []
    for name, (src, _, extra) in UNITS.items():
        obj = os.path.join(OBJ, name + ".o")
        flags = FLAGS + extra
        if force or _stale(obj, unit_deps(name), flags):
            todo.append((name, flags, [cc] + flags + ["-c", os.path.join(CSRC, src), "-o", obj + pid]))
    relink = bool(todo) or not os.path.exists(OUT)
    todo_vario = []
    for name, (src, _) in UNITS_VARIO.items():
        obj = os.path.join(OBJ, name + ".o")
        if force or _stale(obj, vario_deps(name), FLAGS):
            todo_vario.append((name, FLAGS, [cc] + FLAGS + ["-c", os.path.join(CSRC, src), "-o", obj + pid]))
    todo_vario3 = []
    for name, (src, _) in UNITS_VARIO3.items():
        obj = os.path.join(OBJ, name + ".o")
        if force or _stale(obj, vario3_deps(name), FLAGS):
            todo_vario3.append((name, FLAGS, [cc] + FLAGS + ["-c", os.path.join(CSRC, src), "-o", obj + pid]))
    todo_lik = []
    for name, (src, _) in UNITS_LIK.items():
        obj = os.path.join(OBJ, name + ".o")
        if force or _stale(obj, lik_deps(name), FLAGS):
            todo_lik.append((name, FLAGS, [cc] + FLAGS + ["-c", os.path.join(CSRC, src), "-o", obj + pid]))
    todo_grad = []
    for name, (src, _) in UNITS_GRAD.items():
        obj = os.path.join(OBJ, name + ".o")
        if force or _stale(obj, grad_deps(name), FLAGS):
            todo_grad.append((name, FLAGS, [cc] + FLAGS + ["-c", os.path.join(CSRC, src), "-o", obj + pid]))
    todo_vecchia = []
    for name, (src, _) in UNITS_VECCHIA.items():
        obj = os.path.join(OBJ, name + ".o")
        if force or _stale(obj, vecchia_deps(name), FLAGS):
            todo_vecchia.append((name, FLAGS, [cc] + FLAGS + ["-c", os.path.join(CSRC, src), "-o", obj + pid]))

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

    todo.sort(key=lambda j: -COST.get(j[0].rstrip("0123456789"), 0))
    with ThreadPoolExecutor(max_workers=jobs or min(len(UNITS), os.cpu_count() or 4)) as ex:
        list(ex.map(run, todo + todo_vecchia + todo_vario + todo_vario3 + todo_lik + todo_grad))
    # (-s: no static symbol table -- 90 kB; the C ABI and the kernels' host stubs are dynamic symbols, `nm -D` lists them)
    links = []
    if relink or _stale(OUT, all_sources()):
        links.append((OUT, [os.path.join(OBJ, n + ".o") for n in UNITS], ["-ldl", "-Wl,-s"]))
    if todo_vario or _stale(OUT_VARIO, [d for n in UNITS_VARIO for d in vario_deps(n)]):
        links.append((OUT_VARIO, [os.path.join(OBJ, n + ".o") for n in UNITS_VARIO], ["-Wl,-s"]))
    if todo_vario3 or _stale(OUT_VARIO3, [d for n in UNITS_VARIO3 for d in vario3_deps(n)]):
        links.append((OUT_VARIO3, [os.path.join(OBJ, n + ".o") for n in UNITS_VARIO3], ["-Wl,-s"]))
    if todo_lik or _stale(OUT_LIK, [d for n in UNITS_LIK for d in lik_deps(n)]):
        links.append((OUT_LIK, [os.path.join(OBJ, n + ".o") for n in UNITS_LIK], ["-Wl,-s"]))
    if todo_grad or _stale(OUT_GRAD, [d for n in UNITS_GRAD for d in grad_deps(n)]):
        links.append((OUT_GRAD, [os.path.join(OBJ, n + ".o") for n in UNITS_GRAD], ["-Wl,-s"]))
    if todo_vecchia or _stale(OUT_VECCHIA, [d for n in UNITS_VECCHIA for d in vecchia_deps(n)]):
        links.append((OUT_VECCHIA, [os.path.join(OBJ, n + ".o") for n in UNITS_VECCHIA], ["-Wl,-s"]))
    for out, objs, tail in links:
        link = [cc, "--offload-arch=gfx950", "-shared", "-fPIC"] + objs + ["-o", out + pid] + tail
        if verbose:
            print(" ".join(link), flush=True)
        subprocess.run(link, check=True)
        os.replace(out + pid, out)
    return OUT


if __name__ == "__main__":
    j = int(sys.argv[sys.argv.index("-j") + 1]) if "-j" in sys.argv else None
    print(build_library(force="--force" in sys.argv, verbose=True, jobs=j))
