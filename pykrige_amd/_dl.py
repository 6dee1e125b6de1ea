"""What the ctypes bindings of the package's shared objects have in common: opening a library, the error mapping, the device number.

Every binding module (_lib, variography, variography3d, likelihood, vecchia, vecchia_grad) keeps its own LIB_PATH, ABI_VERSION, SIGNATURES and cached
``_lib`` and hands them over at call time; nothing of a library is known here."""
import ctypes as C
import os


def open_library(path, prefix, abi_version, signatures):
    """dlopen ``path`` and declare ``signatures`` (name -> (restype, argtypes)).  Raises ImportError if the file is missing, or if it
    is stale: no ``<prefix>_abi_version``, another version than ``abi_version``, or a missing export."""
    if not os.path.exists(path):
        raise ImportError(
            "pykrige_amd: %s is missing -- build it with `python -m pykrige_amd.build` "
            "(needs hipcc; there is no CPU fallback)" % path)
    lib = C.CDLL(path)
    # the version first: a library from before a symbol was added must end in the "rebuild it" message, not in a bare AttributeError
    have = getattr(lib, prefix + "_abi_version", None)
    version = None
    if have is not None:
        have.restype, have.argtypes = signatures[prefix + "_abi_version"]
        version = have()
    stale = "pykrige_amd: %s %%s, this package was written against ABI version %d -- rebuild it (`python -m pykrige_amd.build --force`)" % (
        path, abi_version)
    if version != abi_version:
        raise ImportError(stale % ("has no %s_abi_version" % prefix if version is None else "has ABI version %d" % version))
    for name, (res, args) in signatures.items():
        try:
            fn = getattr(lib, name)
        except AttributeError:
            raise ImportError(stale % ("does not export %s" % name)) from None
        fn.restype = res
        fn.argtypes = args
    return lib


def raise_for(lib, prefix, libname, rc, einval):
    """A failed call's return code as an exception with the library's reason: ValueError for ``einval``, else RuntimeError."""
    msg = (getattr(lib, prefix + "_last_error")() or b"").decode("utf-8", "replace")
    if rc == einval:
        raise ValueError(msg)
    raise RuntimeError("%s: %s (code %d)" % (libname, msg, rc))


def device():
    return int(os.environ.get("MIK_DEVICE", os.environ.get("LOCAL_RANK", "0")))
