"""pykrige_amd -- the PyKrige execute() hot path on AMD MI355X (gfx950).

Drop-in for ``OrdinaryKriging / UniversalKriging / OrdinaryKriging3D / UniversalKriging3D .execute``:
kriging-matrix assembly, dense inverse, per-point right-hand sides and the z / sigma^2 contraction run
as hand-written HIP kernels in ``libmikrige.so`` (C ABI: include/mikrige.h), called through ctypes.
"""
from .kriging import OrdinaryKriging, OrdinaryKriging3D, UniversalKriging, UniversalKriging3D  # noqa: F401
from . import _lib, core, variogram_models  # noqa: F401
from . import variography  # noqa: F401  (directional semivariograms and variogram maps: libmikvario.so, loaded on first use)
from . import variography3d  # noqa: F401  (the same tools for the 3-D classes: libmikvario3.so, loaded on first use)
from . import likelihood  # noqa: F401  (ML / REML fit of the variogram and its anisotropy: libmiklik.so, loaded on first use)
from . import vecchia  # noqa: F401  (the same fit under Vecchia's approximation, past the N x N matrix: libmikvecchia.so, loaded on first use)
from ._lib import set_devices  # noqa: F401  (single-process multi-GPU: handles span n GPUs; MIK_NGPU does the same)
from . import kriging_tools as kt  # noqa: F401  (the reference's alias)
from . import ok, ok3d, uk, uk3d  # noqa: F401,E402  (`import pykrige; pykrige.ok.OrdinaryKriging` works upstream: pykrige/__init__.py:44-48 binds the submodules)

__all__ = ["OrdinaryKriging", "UniversalKriging", "OrdinaryKriging3D", "UniversalKriging3D", "kt", "ok", "uk", "ok3d", "uk3d", "kriging_tools", "variography", "variography3d", "likelihood", "vecchia", "vecchia_grad", "__version__"]
__version__ = "0.1.0"


def __getattr__(name):
    # vecchia_grad (Vecchia's objective with its analytic gradient and an L-BFGS-B fit: libmikvgrad.so) is imported on first use, not
    # with the package: a process that never asks for it runs none of it
    if name == "vecchia_grad":
        import importlib

        return importlib.import_module(".vecchia_grad", __name__)
    raise AttributeError("module %r has no attribute %r" % (__name__, name))
