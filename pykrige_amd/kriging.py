"""Host-side mirror of the reference's kriging classes for the execute() path.

Same class names, constructor keywords, ``execute`` signatures, return shapes and exceptions as
PyKrige 1.7.3 (/root/reference/src/pykrige: ok.py:187-206,760-1020; uk.py:220-244,1090-1328;
ok3d.py:198-219,735-932; uk3d.py:215-239,877-1146).  Everything between
``a = self._get_kriging_matrix(n)`` and ``return zvalues, sigmasq`` runs on the MI355X through
libmikrige.so (include/mikrige.h); this module only does the front/back matter the reference does in
Python: argument checks, meshgrid order, mask transposition, anisotropy adjustment, host-evaluated
drift terms, output shaping.

``backend``: the reference's values 'vectorized', 'loop' (and 'C' for OrdinaryKriging) are accepted
and all run the same device path -- they keep only their return-type convention ('vectorized' returns
MaskedArrays in every style, the others plain ndarrays unless style='masked').  'hip' is an explicit
alias with the 'loop'/'C' convention.  There is no CPU path in this package.
"""
import contextlib
import os as _os
import warnings

import numpy as np

from . import _lib
from . import core
from . import variogram_models


@contextlib.contextmanager
def _singular_as(backend):
    """A singular local system as the reference's backend reports it: lib/cok.pyx:176-177 ('C') raises ValueError('Singular matrix'),
    scipy.linalg.solve (the others) LinAlgError."""
    try:
        yield
    except np.linalg.LinAlgError as e:
        if backend == "C":
            raise ValueError("Singular matrix") from e
        raise


class _Cols:
    """The coordinate arrays of style='points' as they came (float64, one array per axis), behind the two-dimensional indexing the
    rest of this module uses on an (n, d) point array: cols[:, k], cols[rows, k], cols[slice], cols.shape.  Nothing is copied: the
    library reads the caller's arrays (it stages them in page-locked memory itself) -- the reference's np.array(..., copy=True)
    (ok.py:872-873) protects arrays it goes on to modify; these are only read."""

    __slots__ = ("cols", "shape")

    def __init__(self, cols):
        self.cols = []
        for c in cols:  # read-only VIEWS of the caller's arrays: an accidental in-place write raises instead of reaching user data
            c = c.view()
            c.flags.writeable = False
            self.cols.append(c)
        self.shape = (self.cols[0].shape[0], len(self.cols))

    def __getitem__(self, key):
        if isinstance(key, tuple):
            rows, k = key
            return self.cols[k][rows]
        return _Cols([c[key] for c in self.cols])

    def __array__(self, dtype=None, copy=None):  # np.asarray(cols): the (n, d) array (a copy; nothing on the execute path asks for it)
        if copy is False:  # NumPy 2 protocol: a caller that forbids copying cannot be served (the columns are separate arrays)
            raise ValueError("the (n, d) array of a point list is always a copy")
        a = np.stack(self.cols, axis=1)
        return a if dtype is None else a.astype(dtype, copy=False)


class _Pts:
    """The prediction points of one execute(): adjusted coordinate arrays (style='points', or a grid whose drift callables
    need the adjusted coordinates on the host), or a grid described by its axes and generated on the device (mik_set_grid:
    the meshgrid and the anisotropy adjustment of ok.py:863-885 never exist on the host)."""

    __slots__ = ("arrays", "axes", "center", "rot", "stretch", "mask", "extra", "shape", "npt", "raw")

    def __init__(self, shape, mask, extra, arrays=None, axes=None, center=None, rot=None, stretch=None, raw=False):
        self.shape, self.mask, self.extra = shape, mask, extra
        self.arrays, self.axes, self.center, self.rot, self.stretch = arrays, axes, center, rot, stretch
        self.raw = raw  # `arrays` are the coordinates as given: the device applies center / rot / stretch (mik_adjust_points)
        self.npt = int(np.prod(shape))

    def load(self, h, ndim, cell_range=None, with_extra=True):
        """H2D (arrays) or device-side generation (grid) of the points, optionally only cells [first, first + count).  The library
        stages host arrays synchronously (mik_set_points returns after its copy into page-locked memory): views of the caller's
        arrays (_Cols) are not referenced after this call returns, and must not be if the upload ever becomes asynchronous."""
        extra = self.extra if with_extra else None
        if cell_range is None:
            mask = self.mask
        else:
            sl = slice(cell_range[0], cell_range[0] + cell_range[1])
            mask = None if self.mask is None else self.mask[sl]
            extra = None if extra is None else np.ascontiguousarray(extra[:, sl])
        if self.axes is not None:
            h.set_grid(self.axes, self.center, self.rot, self.stretch, mask=mask, extra_rows=extra, cell_range=cell_range)
            return
        a = self.arrays if cell_range is None else self.arrays[sl]
        h.set_points(a[:, 0], a[:, 1], a[:, 2] if ndim == 3 else None, mask=mask, extra_rows=extra)
        if self.raw:
            h.adjust_points(self.center, self.rot, self.stretch)


class _KrigingBase:
    eps = 1.0e-10  # ok.py:177, uk.py:210
    UNBIAS = True  # uk.py:208
    # ok.py:178-185: the named models as functions (m, d) -> gamma; what `variogram_function` is for a named model.  The device
    # evaluates them itself (variogram_model selects the kernel); the functions are for callers that plot or inspect the fit.
    variogram_dict = {
        "linear": variogram_models.linear_variogram_model,
        "power": variogram_models.power_variogram_model,
        "gaussian": variogram_models.gaussian_variogram_model,
        "spherical": variogram_models.spherical_variogram_model,
        "exponential": variogram_models.exponential_variogram_model,
        "hole-effect": variogram_models.hole_effect_variogram_model,
    }
    _ndim = 2
    _universal = False
    _backends = ("vectorized", "loop", "hip")
    _label = "kriging"

    # ---------------------------------------------------------------- construction helpers
    def _init_common(self, variogram_model, variogram_parameters, variogram_function, exact_values, pseudo_inv,
                     pseudo_inv_type, verbose, enable_plotting):
        self.pseudo_inv = bool(pseudo_inv)
        self.pseudo_inv_type = str(pseudo_inv_type)
        if self.pseudo_inv_type not in ("pinv", "pinvh"):  # core.py:33 P_INV keys
            raise ValueError("pseudo inv type not valid: " + str(pseudo_inv_type))
        self.model = None
        if hasattr(variogram_model, "pykrige_kwargs"):
            # a GSTools CovModel (ok.py:223-239): it becomes a custom variogram; its anisotropy is taken by the caller
            self.model = variogram_model
            variogram_model, variogram_function, variogram_parameters = "custom", variogram_model.pykrige_vario, []
        self.variogram_model = variogram_model
        self.variogram_function = None
        if variogram_model == "custom":
            if variogram_function is None or not callable(variogram_function):
                raise ValueError("Must specify callable function for custom variogram model.")
            self.variogram_function = variogram_function  # evaluated on the host (it is Python), geometry stays on the device
        elif variogram_model not in core.MODELS:
            raise ValueError("Specified variogram model '%s' is not supported." % variogram_model)
        else:
            self.variogram_function = self.variogram_dict[variogram_model]  # ok.py:253
        if not isinstance(exact_values, bool):
            raise ValueError("exact_values has to be boolean True or False")
        self.exact_values = exact_values
        self.verbose = verbose
        self.enable_plotting = enable_plotting
        if self.enable_plotting and self.verbose:
            print("Plotting Enabled\n")
        self._user_parameters = variogram_parameters
        self._handle = None
        return variogram_parameters

    def _set_variogram_parameters(self, variogram_parameters, nlags, weight, updating=False):
        if self.verbose:  # (verbose=True narrates what upstream narrates, line for line: ok.py:310-375, 488-553 and the three siblings)
            print("Updating variogram mode..." if updating else "Initializing variogram model...")
        plist = core.make_variogram_parameter_list(self.variogram_model, variogram_parameters)
        fitted = plist is None
        if plist is None:
            from . import variogram_fit  # constructor-time only; never on the execute() path

            self.lags, self.semivariance, plist = variogram_fit.fit(
                self._coords_adj, self._values(), self.variogram_model, nlags, weight,
                getattr(self, "coordinates_type", "euclidean"), binned=self._device_variogram(nlags))
        else:  # the reference bins the experimental variogram even when parameters are given; here on first use
            self.__dict__.pop("lags", None)
            self.__dict__.pop("semivariance", None)
        self._nlags = nlags
        for name in self._LAZY_STATS:  # a new variogram invalidates the statistics
            if self.__dict__.get(name, 0) is not None:
                self.__dict__.pop(name, None)
        # a FITTED parameter set is the least-squares solution as it comes, an ndarray (core.py:575-627 returns res.x); a given one is a list (core.py:353-357)
        self.variogram_model_parameters = np.array([float(v) for v in plist]) if fitted else [float(v) for v in plist]
        if self.verbose:
            par = self.variogram_model_parameters
            if type(self) is OrdinaryKriging:
                print("Coordinates type: '%s'" % self.coordinates_type, "\n")
            if self.variogram_model == "linear":
                print("Using '%s' Variogram Model" % "linear")
                print("Slope:", par[0])
                print("Nugget:", par[1], "\n")
            elif self.variogram_model == "power":
                print("Using '%s' Variogram Model" % "power")
                print("Scale:", par[0])
                print("Exponent:", par[1])
                print("Nugget:", par[2], "\n")
            elif self.variogram_model == "custom":
                print("Using Custom Variogram Model")
            else:
                print("Using '%s' Variogram Model" % self.variogram_model)
                print("Partial Sill:", par[0])
                print("Full Sill:", par[0] + par[2])
                print("Range:", par[1])
                print("Nugget:", par[2], "\n")
        if getattr(self, "enable_plotting", False):  # ok.py:355-356, 534-535
            self.display_variogram_model()
        if self.verbose:
            print("Calculating statistics on variogram model fit...")
            # upstream computes them here (always in update_variogram_model and in the UK / 3-D constructors, on request in OrdinaryKriging's) and
            # prints them; without verbose they stay lazy (_LAZY_STATS)
            if updating or type(self) is not OrdinaryKriging or getattr(self, "_enable_statistics", False):
                self._compute_statistics()

    def _device_variogram(self, nlags):
        """Experimental semivariogram on the GPU (mik_experimental_variogram) when one is visible and the O(N^2) pair
        reduction is worth a launch; None -> the caller bins on the host with SciPy (same numbers to 1e-12).  This is
        constructor-time work, outside the execute() path, so a host route is legitimate here."""
        if self._values().size < int(_os.environ.get("MIK_DEVICE_VARIOGRAM_MIN_N", "512")) or nlags > 64:
            return None
        try:
            if _lib.load().mik_device_count() < 1:
                return None
        except ImportError:
            return None
        h = self._get_handle()
        self._factor_key = None
        ca = self._coords_adj
        h.set_problem(ndim=self._ndim, xs=ca[:, 0], ys=ca[:, 1], zs=ca[:, 2] if self._ndim == 3 else None,
                      values=self._values(), model_id=0, params=[1.0, 0.0],
                      geographic=getattr(self, "coordinates_type", "euclidean") == "geographic")
        return h.experimental_variogram(nlags)

    def _update_variogram_model(self, variogram_model, variogram_parameters, variogram_function, nlags, weight, anisotropy):
        """Body shared by the four update_variogram_model signatures (ok.py:379-545, uk.py:630-760, ok3d.py:368-520,
        uk3d.py:452-600) without the statistics pass, which execute() never reads.  As in the reference the anisotropy
        keywords DEFAULT to isotropic: omitting them resets the object to scaling 1 / angle 0 and re-adjusts the stations
        (UniversalKriging's point_log wells keep their construction-time adjustment -- the reference does not touch them)."""
        self.model = None
        if hasattr(variogram_model, "pykrige_kwargs"):  # GSTools CovModel: its own anisotropy (ok.py:430-444, ok3d.py:432-445)
            self.model = variogram_model
            if self._ndim == 2:
                if self.model.field_dim == 3:
                    raise ValueError("GSTools: model dim is not 1 or 2")
                if self.model.latlon and getattr(self, "coordinates_type", "euclidean") == "euclidean":
                    raise ValueError("GSTools: latlon models require geographic coordinates")
                anisotropy = dict(anisotropy_scaling=self.model.pykrige_anis, anisotropy_angle=self.model.pykrige_angle)
            else:
                if self.model.field_dim < 3:
                    raise ValueError("GSTools: model dim is not 3")
                anisotropy = dict(anisotropy_scaling_y=self.model.pykrige_anis_y, anisotropy_scaling_z=self.model.pykrige_anis_z,
                                  anisotropy_angle_x=self.model.pykrige_angle_x, anisotropy_angle_y=self.model.pykrige_angle_y,
                                  anisotropy_angle_z=self.model.pykrige_angle_z)
            variogram_model, variogram_function, variogram_parameters = "custom", variogram_model.pykrige_vario, []
        if variogram_model == "custom":
            if variogram_function is None or not callable(variogram_function):
                raise ValueError("Must specify callable function for custom variogram model.")
            self.variogram_function = variogram_function
        elif variogram_model not in core.MODELS:
            raise ValueError("Specified variogram model '%s' is not supported." % variogram_model)
        else:
            self.variogram_function = self.variogram_dict[variogram_model]
        self.variogram_model = variogram_model
        if getattr(self, "coordinates_type", "euclidean") == "geographic":
            if anisotropy.get("anisotropy_scaling", 1.0) != 1.0 and anisotropy["anisotropy_scaling"] != self.anisotropy_scaling:
                warnings.warn("Anisotropy is not compatible with geographic coordinates. Ignoring user set anisotropy.",
                              UserWarning)  # ok.py:478-487
        elif any(v != getattr(self, k) for k, v in anisotropy.items()):
            if self.verbose:
                print("Adjusting data for anisotropy...")
            for k, v in anisotropy.items():
                setattr(self, k, v)
            self._adjust_stations()
        self._set_variogram_parameters(variogram_parameters, nlags, weight, updating=True)

    def update_variogram_model(self, variogram_model, variogram_parameters=None, variogram_function=None, nlags=6,
                               weight=False, anisotropy_scaling=1.0, anisotropy_angle=0.0):
        """Changes the variogram model and the anisotropy (ok.py:379-387, uk.py:630-639: same signature, same defaults)."""
        self._update_variogram_model(variogram_model, variogram_parameters, variogram_function, nlags, weight,
                                     dict(anisotropy_scaling=anisotropy_scaling, anisotropy_angle=anisotropy_angle))

    # ---------------------------------------------------------------- device plumbing
    def _get_handle(self):
        if self._handle is None:
            self._handle = _lib.acquire_handle()  # a parked one if there is (mik_create + mik_destroy: 20 - 30 ms; _lib.release_handle)
        return self._handle

    _max_points = 0  # most points one call of this object handed to its handle
    _max_fields = 0  # most fields one execute_fields call of this object handed to its handle

    def _handle_bytes(self):
        """Device memory the handle holds at most after this object's calls, for the parking rule: matrix, its probe copy and panels (3 Mp^2) + the
        right-hand sides of two launches of <= 131 072 points (2 npt Mp) + stations and results."""
        n = int(np.size(self._values())) + 16
        mp = -(-n // 128) * 128
        npt = min(int(self._max_points), 131072)
        nf = self._max_fields + 16  # execute_fields: the fields, their coefficients and their z planes
        return 8.0 * (3.0 * mp * mp + 2.0 * npt * mp + 8.0 * self._max_points + 8.0 * n
                      + (nf * (mp + n + self._max_points) if self._max_fields else 0.0))

    def __getstate__(self):
        """Pickling / copy.deepcopy (sklearn's clone, joblib workers, cached models): upstream's objects are plain Python attributes and travel; here the
        device side -- the library handle and the note of what is factored in it -- stays behind and the copy builds its own on its first execute()."""
        state = dict(self.__dict__)
        state["_handle"] = None
        state.pop("_factor_key", None)
        return state

    def __del__(self):
        h = self.__dict__.get("_handle")
        if h is not None:
            self._handle = None
            try:
                _lib.release_handle(h, self._handle_bytes())
            except Exception:  # noqa: BLE001  (interpreter shutdown: the handle's own __del__ closes it)
                pass

    def _values(self):
        return self.VALUES if self._ndim == 3 else self.Z

    def _station_extra_cols(self):
        return None

    def _wells(self):
        return None

    def _regional_linear(self):
        return False

    def _set_problem(self, h, with_drift=True, values=None, pseudo_inv=False, exact_values=None, eps=None):
        """H2D of the stations / drift description."""
        self._factor_key = None  # whatever the handle held is replaced
        ca = self._coords_adj
        kw = dict(
            ndim=self._ndim, xs=ca[:, 0], ys=ca[:, 1], zs=ca[:, 2] if self._ndim == 3 else None,
            values=self._values() if values is None else values, model_id=_lib.MODEL_IDS[self.variogram_model],
            params=self.variogram_model_parameters, eps=self.eps if eps is None else eps,
            exact_values=self.exact_values if exact_values is None else exact_values,
            regional_linear=self._regional_linear() if with_drift else False,
            wells=self._wells() if with_drift else None,
            extra_cols=self._station_extra_cols() if with_drift else None,
            geographic=getattr(self, "coordinates_type", "euclidean") == "geographic",
        )
        if self.variogram_model == "custom":
            fn, par = self.variogram_function, self.variogram_model_parameters
            h.set_custom_variogram(lambda d: fn(par, d))
            kw["params"] = [0.0, 0.0, 0.0]
        if self.pseudo_inv and (with_drift or pseudo_inv):
            # ok.py:660-661: a_inv = P_INV[self.pseudo_inv_type](a) -- on the device (mik_problem.pseudo_inv)
            kw["pseudo_inv"] = {"pinv": 1, "pinvh": 2}[self.pseudo_inv_type]
        h.set_problem(**kw)

    def _problem_key(self):
        """Digest of everything mik_set_problem + mik_factor depend on; None = not cacheable (a user callable)."""
        if self.variogram_model == "custom" or _os.environ.get("MIK_FACTOR_CACHE", "1") == "0":
            return None
        import hashlib

        d = hashlib.blake2b(digest_size=16)
        for a in (self._coords_adj, self._values(), self._wells(), self._station_extra_cols()):
            d.update(b"-" if a is None else np.ascontiguousarray(a, dtype=np.float64).tobytes())
        d.update(repr((self._ndim, self.variogram_model, [float(v) for v in self.variogram_model_parameters], float(self.eps),
                       bool(self.exact_values), bool(self._regional_linear()), bool(self.pseudo_inv), self.pseudo_inv_type,
                       getattr(self, "coordinates_type", "euclidean"))).encode())
        return d.digest()

    def _factor_key_for(self, h):
        """The key of this object's problem as factored on handle h: a changed library option (factor path, device group, ...)
        invalidates the factor too.  None = not cacheable."""
        key = self._problem_key()
        return None if key is None else (key, h.option_epoch)

    def _upload_and_factor(self):
        """K1 + K2 on the device (inverse, or pseudo-inverse when pseudo_inv=True).  The reference re-assembles and re-inverts
        the matrix on every execute() (ok.py:898, 663); here the factored matrix stays on the device and is reused while the
        problem (stations, values, variogram, drift set-up) is unchanged -- a second execute() on new points only predicts."""
        h = self._get_handle()
        key = self._factor_key_for(h)
        if key is not None and key == getattr(self, "_factor_key", None):
            self.factor_reused = True
            return h
        self._set_problem(h)
        h.factor()
        self._factor_key = key
        self.factor_reused = False
        return h

    def _solve(self, P):
        h = self._upload_and_factor()
        self._max_points = max(self._max_points, int(np.prod(P.shape)))
        P.load(h, self._ndim)
        h.predict()
        self.last_timing = h.timing()
        return h.get_results()

    def _prepare(self, style, axes, mask, specified_drift_arrays=None, backend="vectorized"):
        """Everything execute() does on the host before the solve -> _Pts.  Grids ('grid' / 'masked') are handed to the
        device as axes + the anisotropy matrices unless a drift callable needs the adjusted coordinates on the host
        (functional drifts) or MIK_DEVICE_GRID=0 asks for the host meshgrid."""
        self._point_dtype = self._narrow_dtype(axes)
        if (style not in ("grid", "masked") or _os.environ.get("MIK_DEVICE_GRID", "1") == "0"
                or getattr(self, "functional_drift", False)):
            # coordinate arrays.  Round 3: they too are adjusted on the device (mik_adjust_points; the host only stacks them) unless
            # a functional drift needs the adjusted coordinates here, the coordinates are geographic (no adjustment at all,
            # ok.py:892-896) or MIK_DEVICE_POINTS=0 asks for the host adjustment
            raw = (not getattr(self, "functional_drift", False) and getattr(self, "coordinates_type", "euclidean") != "geographic"
                   and _os.environ.get("MIK_DEVICE_POINTS", "1") != "0")
            pts, shape, mask, extra = self._prepare_points(style, axes, mask, specified_drift_arrays, backend, adjust=not raw)
            if not raw:
                return _Pts(shape, mask, extra, arrays=pts)
            rot, stretch = core.anisotropy_matrices(self._ndim, self._scaling(), self._angle())
            return _Pts(shape, mask, extra, arrays=self._as_centred(pts), center=self._center(), rot=rot, stretch=stretch, raw=True)
        axes, shape, mask = self._grid_from(style, axes, mask)
        extra = self._grid_rows(style, axes, shape, mask, specified_drift_arrays, backend)
        if getattr(self, "coordinates_type", "euclidean") == "geographic":
            return _Pts(shape, mask, extra, axes=axes)  # no anisotropy correction in spherical coordinates (ok.py:892-896)
        rot, stretch = core.anisotropy_matrices(self._ndim, self._scaling(), self._angle())
        return _Pts(shape, mask, extra, axes=self._as_centred(axes), center=self._center(), rot=rot, stretch=stretch)

    _point_dtype = None

    def _narrow_dtype(self, axes):
        """The reference never casts the prediction coordinates (ok.py:849-850: np.array(xpoints, copy=True)) and centres them IN PLACE
        (core.py:146 `X -= center`, X = np.vstack of the coordinate arrays): when every array is float32 (or float16) the centred
        coordinates are rounded to that type -- 1e-7 relative, 1.7e-7 on z in the differential run of scripts/edge_forms_vs_reference.py --
        before the rotation continues in float64.  Returns that dtype, or None when the arrays promote to float64 (integer arrays: the
        reference's in-place subtract raises UFuncTypeError; here they are kriged as float64).  Geographic coordinates are not centred."""
        if getattr(self, "coordinates_type", "euclidean") == "geographic":
            return None
        try:
            rt = np.result_type(*[a.dtype if isinstance(a, np.ndarray) else np.asarray(a).dtype for a in axes])
        except Exception:  # noqa: BLE001  (ragged / object input: the float64 cast that follows raises what it raises)
            return None
        return rt if rt.kind == "f" and rt.itemsize < 8 else None

    def _as_centred(self, pts, nd="points"):
        """pts (float64: a list of axes, an (n, d) array or _Cols) as the reference's narrower in-place centring leaves them:
        x -> float64(narrow(x - c)) + c.  (The `+ c`, undone by the adjustment's own `- c`, costs an ulp of float64: nine orders below the effect.)
        nd: the narrow dtype (default: the one of this call's prediction points, _narrow_dtype)."""
        if isinstance(nd, str):
            nd = self._point_dtype
        if nd is None:
            return pts
        cen = self._center()
        if isinstance(pts, list):
            return [(a - c).astype(nd).astype(np.float64) + c for a, c in zip(pts, cen)]
        cols = [(np.asarray(pts[:, k]) - c).astype(nd).astype(np.float64) + c for k, c in enumerate(cen)]
        return _Cols(cols) if isinstance(pts, _Cols) else np.stack(cols, axis=1)

    def _grid_rows(self, style, axes, shape, mask, specified_drift_arrays, backend):
        return None  # host-evaluated drift rows of a grid: universal kriging only

    def _prepare_points(self, style, axes, mask, specified_drift_arrays=None, backend="vectorized", adjust=True):
        """Everything execute() does on the host before the solve: returns (pts_adj, shape, mask, extra_rows); adjust=False
        leaves the anisotropy adjustment of the coordinates to the device (mik_adjust_points)."""
        pts, shape, mask = self._points_from(style, axes, mask, columns=not adjust)
        if getattr(self, "coordinates_type", "euclidean") == "geographic" or not adjust:
            return pts, shape, mask, None  # no anisotropy correction in spherical coordinates (ok.py:892-896)
        return core.adjust_for_anisotropy(self._as_centred(pts), self._center(), self._scaling(), self._angle()), shape, mask, None

    # ---------------------------------------------------------------- variogram-fit statistics (core.py:759-851)
    _LAZY_STATS = ("delta", "sigma", "epsilon", "Q1", "Q2", "cR")

    def _compute_statistics(self):
        """_find_statistics on the device (mik_statistics): station i kriged from stations 0..i-1 with the ORDINARY
        system (core._krige ignores drift terms), then delta / sigma / epsilon and Q1, Q2, cR as the reference."""
        h = self._get_handle()
        y = self._values()
        if self.pseudo_inv:
            # core.py:749-750: lstsq per growing subset (duplicated stations); no recursion exists for singular leading
            # systems, so each station is kriged through the device pseudo-inverse (core._statistics_pseudo_inv).
            # N - 1 small factorisations: on ONE device (a device group would exchange every one of them), and with the
            # rule core._krige applies whatever the object's exact_values says -- b is zeroed at the coincident station with
            # the fixed tolerance 1e-10 (core.py:728-745).
            full = self._coords_adj
            if h.n_devices > 1:
                h = _lib.Handle(h.device)
                h.set_devices(1)

            def subset(i):
                self._coords_adj = full[:i]
                try:
                    self._set_problem(h, with_drift=False, values=y[:i], pseudo_inv=True, exact_values=True, eps=1e-10)
                finally:
                    self._coords_adj = full

            par = self.variogram_model_parameters
            gamma = ((lambda d: self.variogram_function(par, d)) if self.variogram_model == "custom"
                     else (lambda d: core.variogram_value(self.variogram_model, par, d)))
            try:
                k, ss = core._statistics_pseudo_inv(h, subset, full, y, gamma,
                                                    getattr(self, "coordinates_type", "euclidean") == "geographic")
            finally:
                if h is not self._get_handle():
                    h.close()
                self._factor_key = None
        else:
            self._set_problem(h, with_drift=False)
            k, ss = h.statistics(y.size)
        self.delta, self.sigma = core._delta_sigma(y, k, ss, self.eps)
        self.epsilon = self.delta / self.sigma
        self.Q1 = abs(np.sum(self.epsilon) / (self.epsilon.shape[0] - 1))
        self.Q2 = np.sum(self.epsilon**2) / (self.epsilon.shape[0] - 1)
        self.cR = self.Q2 * np.exp(np.sum(np.log(self.sigma**2)) / self.sigma.shape[0])
        if self.verbose:
            print("Q1 =", self.Q1)
            print("Q2 =", self.Q2)
            print("cR =", self.cR, "\n")

    def __getattr__(self, name):
        # UK / 3-D constructors of the reference run _find_statistics unconditionally (uk.py:380, ok3d.py:352,
        # uk3d.py:380); here the same attributes are computed on first use instead of at construction.
        if name in _KrigingBase._LAZY_STATS and "_handle" in self.__dict__:
            self._compute_statistics()
            return self.__dict__[name]
        if name in ("lags", "semivariance") and "_coords_adj" in self.__dict__:
            from . import variogram_fit

            nl = self.__dict__.get("_nlags", 6)
            binned = self._device_variogram(nl)
            self.lags, self.semivariance = binned if binned is not None else variogram_fit.experimental_variogram(
                self._coords_adj, self._values(), nl, getattr(self, "coordinates_type", "euclidean"))
            return self.__dict__[name]
        raise AttributeError(name)

    def get_epsilon_residuals(self):
        return self.epsilon

    def get_statistics(self):
        return self.Q1, self.Q2, self.cR

    def print_statistics(self):
        print("Q1 =", self.Q1)
        print("Q2 =", self.Q2)
        print("cR =", self.cR)

    def get_variogram_points(self):
        """(lags, variogram model evaluated at the lags) -- ok.py:569-587."""
        if self.variogram_model == "custom":
            return self.lags, self.variogram_function(self.variogram_model_parameters, self.lags)
        return self.lags, core.variogram_value(self.variogram_model, self.variogram_model_parameters, self.lags)

    def display_variogram_model(self):
        """Binned semivariances and the model curve (ok.py:555-567); needs matplotlib."""
        import matplotlib.pyplot as plt

        lags, model = self.get_variogram_points()
        ax = plt.figure().add_subplot(111)
        ax.plot(lags, self.semivariance, "r*")
        ax.plot(lags, model, "k-")
        plt.show()

    def plot_epsilon_residuals(self):
        """Scatter of the variogram-fit epsilon residuals (ok.py:601-609); needs matplotlib."""
        import matplotlib.pyplot as plt

        eps = self.epsilon
        ax = plt.figure().add_subplot(111)
        ax.scatter(range(eps.size), eps, c="k", marker="*")
        ax.axhline(y=0.0)
        plt.show()

    def _get_kriging_matrix(self, n=None, n_withdrifts=None):
        """The kriging matrix as the reference's method of the same name returns it (ok.py:626-648, uk.py:861-920,
        3-D twins), assembled by K1 on the device and copied back -- for inspection; execute() never brings it to the host.
        (n, and n_withdrifts of the universal classes, are upstream's positional arguments: the station count and the count with drift
        columns -- both follow from the object and are accepted for the call's sake.)"""
        h = self._get_handle()
        self._set_problem(h)
        h.assemble_only()
        return h.get_matrix(0)

    def switch_verbose(self):
        self.verbose = not self.verbose

    def switch_plotting(self):
        self.enable_plotting = not self.enable_plotting

    # ---------------------------------------------------------------- execute front / back matter
    _mw_backends = ()  # backends the reference accepts together with n_closest_points

    def _check_backend(self, backend, n_closest_points):
        if n_closest_points is not None and n_closest_points <= 1:
            raise ValueError("n_closest_points has to be at least two!")  # ok.py:837-840
        if backend not in self._backends:
            raise ValueError("Specified backend {} is not supported for {}.".format(backend, self._label))
        if n_closest_points is not None and backend not in self._mw_backends:
            raise ValueError("Specified backend {} for a moving window is not supported.".format(backend))  # ok.py:982-986

    def _solve_moving_window(self, P, n_closest_points, backend):
        """cKDTree.query + _exec_loop_moving_window / _c_exec_loop_moving_window on the device."""
        h = self._get_handle()
        self._set_problem(h)
        self._max_points = max(self._max_points, int(np.prod(P.shape)))
        P.load(h, self._ndim, with_extra=False)
        with _singular_as(backend):
            h.predict_moving_window(int(n_closest_points))
        self.last_timing = h.timing()
        return h.get_results()

    def _grid_from(self, style, axes, mask):
        """Axes cast to fp64, output shape and the flattened mask of style='grid' / 'masked' (ok.py:849-862, 896;
        ok3d.py:841-861, 893) -- the checks of the reference without its meshgrid."""
        # the reference does not cast (integer grids crash in its in-place subtract); cast to fp64 here
        axes = [np.atleast_1d(np.squeeze(np.array(a, copy=True, dtype=np.float64))) for a in axes]
        sizes = [a.size for a in axes]
        shape = tuple(reversed(sizes))  # (ny, nx) / (nz, ny, nx)
        if style == "masked":
            if mask is None:
                raise IOError("Must specify boolean masking array when style is 'masked'.")
            mask = np.asarray(mask)
            if self._ndim == 3 and mask.ndim != 3:
                raise ValueError("Mask is not three-dimensional.")
            if mask.ndim != self._ndim:
                raise ValueError("Mask dimensions do not match specified grid dimensions.")
            if mask.shape != shape:
                if mask.shape == tuple(sizes):
                    mask = mask.T if self._ndim == 2 else mask.swapaxes(0, 2)
                else:
                    raise ValueError("Mask dimensions do not match specified grid dimensions.")
            mask = mask.flatten().astype(bool)
        else:
            mask = None  # ok.py:896 / ok3d.py:893: `if style != "masked": mask = np.zeros(npt, dtype="bool")` -- a mask handed
            # to style="grid" is ignored, every cell is kriged
        return axes, shape, mask

    def _meshgrid(self, axes):
        """The reference's flattened meshgrid (ok.py:863-867, ok3d.py:866-870) as an (npt, d) array."""
        if self._ndim == 2:
            gx, gy = np.meshgrid(axes[0], axes[1])
            return np.stack((gx.ravel(), gy.ravel()), axis=1)
        gz, gy, gx = np.meshgrid(axes[2], axes[1], axes[0], indexing="ij")
        return np.stack((gx.ravel(), gy.ravel(), gz.ravel()), axis=1)

    def _points_from(self, style, axes, mask, columns=False):
        """Reference meshgrid order and mask handling (ok.py:849-878; ok3d.py:841-876).  columns=True (style='points' whose
        coordinates go to the device raw): the coordinate arrays stay the caller's (_Cols: no host copy of npt x d doubles;
        round 3 made one F-ordered copy, rounds 1-2 two copies)."""
        if style != "grid" and style != "masked" and style != "points":
            raise ValueError("style argument must be 'grid', 'points', or 'masked'")
        if style in ("grid", "masked"):
            axes, shape, mask = self._grid_from(style, axes, mask)
            pts = self._meshgrid(axes)
        else:
            # columns (the coordinates go to the device as they are): no host copy at all -- views of the caller's arrays (_Cols)
            axes = [np.atleast_1d(np.squeeze(np.asarray(a, dtype=np.float64) if columns else np.array(a, copy=True, dtype=np.float64)))
                    for a in axes]
            sizes = [a.size for a in axes]
            if len(set(sizes)) != 1:
                raise ValueError("xpoints and ypoints%s must have same dimensions when treated as listing "
                                 "discrete points." % (", zpoints" if self._ndim == 3 else ""))
            if any(a.ndim > 1 for a in axes):
                # the reference stacks xpts[:, np.newaxis] columns (ok.py:886-888) and hands them to cdist, which refuses anything but (n, d)
                raise ValueError("XB must be a 2-dimensional array.")
            shape = (sizes[0],)
            if columns:
                pts = _Cols([a.reshape(-1) for a in axes])
            else:
                pts = np.stack(axes, axis=1)
            mask = None
        return pts, shape, mask

    def _finish(self, z, ss, style, shape, mask, backend):
        if style == "masked":
            z = np.ma.array(z, mask=mask)
            ss = np.ma.array(ss, mask=mask)
        elif backend == "vectorized" and z.size:
            # reference quirk: _exec_vector returns MaskedArrays (all-False mask) in every style (an EMPTY point list comes back as plain arrays)
            z = np.ma.array(z, mask=np.zeros(z.shape, dtype=bool))
            ss = np.ma.array(ss, mask=np.zeros(ss.shape, dtype=bool))
        return z.reshape(shape), ss.reshape(shape)

    # ---------------------------------------------------------------- several value fields on one station set (mik_set_fields)
    _FIELDS_DOC = """Krige F value fields measured at this object's stations in one call.

        ``values`` is array-like of shape (N, F), one column per field (a 1-D (N,) array is F = 1), cast to float64.  Returns
        ``(zvalues, sigmasq)``: ``zvalues`` has shape ``(F,) + shape`` and ``sigmasq`` ``shape``, where ``shape`` is what
        ``execute()`` returns for the same call; the return types follow ``execute()`` (MaskedArrays for backend 'vectorized' and
        for style 'masked', the mask repeated over the field axis; masked points are 0.0 in every plane).

        The variogram is the object's: it was fitted to (or given with) the object's own values at construction and does not
        change.  ``zvalues[f]`` is what ``execute()`` gives on an object built from the same stations and ``values[:, f]`` with
        ``variogram_parameters`` set explicitly to this object's parameters and every other constructor argument the same
        (drifts, anisotropy, exact_values, pseudo_inv, coordinates_type, custom callables) -- not what F objects that each fit
        their own variogram would give.  sigma^2 does not depend on the values and is computed once.  The matrix, its inverse,
        the right-hand sides and sigma^2 are shared by the fields, so F fields cost little more than one ``execute()``.

        ``OrdinaryKriging`` and ``OrdinaryKriging3D`` also take ``n_closest_points`` (the moving window) with the argument rules of
        their ``execute()``: ``zvalues[f]`` is then bit for bit ``execute(..., n_closest_points=k)`` of such a per-field object, and
        ``sigmasq`` that of this object.  A point's local system does not depend on the values: the neighbour search, the local
        right-hand sides and, for windows up to 256, the factorisation of each local system are shared by up to G - 2 fields per pass
        (G = 4, 8, 16 or 32 with the window).  The universal-kriging classes have no moving window, as in their ``execute()``.

        Missing stations (``valid``, the last keyword; ``None`` is everything described so far, non-finite values included: they
        raise).  ``valid`` is a boolean array of the shape of ``values`` -- ``(N, F)``, or ``(N,)`` for 1-D values -- and True means
        "measured".  Entries of ``values`` where ``valid`` is False are ignored (they may be NaN or inf and are replaced by 0.0 on the
        host); entries where it is True must be finite, and every field needs at least one valid station.  The call then returns
        ``(zvalues, sigmasq)`` with ``sigmasq`` of shape ``(F,) + shape`` under the type rules of ``zvalues``: ``zvalues[f]`` and
        ``sigmasq[f]`` are ``execute()`` of an object built from the stations with ``valid[:, f]`` alone, with this object's
        variogram parameters, drifts, anisotropy, ``exact_values``, centre and adjusted coordinates.  Nothing is factored again: for
        the missing stations ``S`` of a field, ``R`` everything else, ``B`` the one resident inverse, ``b(p)`` the right-hand side of
        point p, ``v0`` the field with zeros at ``S`` and ``c0 = B[:, :N] v0``,
        ``L L^T = B_SS``, ``W = L^-1 B[S, :]``, ``g = L^-1 c0_S``, ``c~ = c0 - W^T g`` (``c~_S = 0``) give
        ``z_R(p) = c~ . b(p)`` and ``sigma^2_R(p) = sigma^2(p) + |W b(p)|^2`` exactly.  Fields with the same ``valid`` column share
        the work and the bits of their ``sigmasq`` plane; a field without gaps costs nothing extra.  A pattern whose ``B_SS`` is not
        numerically positive definite returns NaN in its fields' planes and nothing is raised.  ``pseudo_inv=True`` raises
        ``ValueError`` (the identity needs a regular inverse), ``n_closest_points`` together with ``valid`` raises
        ``NotImplementedError``, and a handle that spans a device group raises ``ValueError``."""

    def _field_gaps(self, values, v, valid, zero=True):
        """valid of execute_fields against the (N, F) values v: the (N, F) boolean array; v gets 0.0 where it is False (zero=False: v stays
        as it is and a field may be empty -- execute_fields_window, whose device path never reads those entries and has a bound of its own)."""
        m = np.asarray(valid)
        if m.dtype != np.bool_:
            raise ValueError("valid must be a boolean array (True = measured); got dtype %s" % m.dtype)
        want = (v.shape[0],) if np.ndim(values) == 1 else v.shape
        if m.shape != want:
            raise ValueError("valid has shape %s; values has shape %s" % (m.shape, want))
        m = m.reshape(v.shape)
        if not np.all(np.isfinite(v[m])):
            raise ValueError("values holds non-finite entries where valid is True")
        if not zero:
            return m
        empty = np.flatnonzero(~m.any(axis=0))
        if empty.size:
            raise ValueError("valid: field %d has no valid station" % int(empty[0]))
        v[~m] = 0.0
        return m

    def _field_values(self, values, valid=None):
        n = int(np.size(self._values()))
        v = np.array(values, copy=True, dtype=np.float64)
        if v.ndim == 1:
            v = v[:, None]
        if v.ndim != 2:
            raise ValueError("values must have shape (N,) or (N, F); got %d dimensions" % v.ndim)
        if v.shape[0] != n:
            raise ValueError("values has %d rows; the object has %d stations" % (v.shape[0], n))
        if v.shape[1] == 0:
            raise ValueError("values holds no field (F = 0)")
        if valid is None and not np.all(np.isfinite(v)):
            raise ValueError("values holds non-finite entries")
        return v

    def _execute_fields(self, style, axes, values, mask, backend, prepare_kw, n_closest_points=None, valid=None):
        """execute_fields of the four classes: every argument is checked on the host before the device is touched."""
        if style != "grid" and style != "masked" and style != "points":
            raise ValueError("style argument must be 'grid', 'points', or 'masked'")
        self._check_backend(backend, n_closest_points)
        v = self._field_values(values, valid)
        gaps = None
        if valid is not None:
            gaps = self._field_gaps(values, v, valid)
            if n_closest_points is not None:
                raise NotImplementedError("execute_fields: valid together with n_closest_points (the moving window with gaps) is not built")
            if self.pseudo_inv:
                raise ValueError("execute_fields with valid needs a regular inverse: the block-inverse identity does not hold for pseudo_inv=True")
            if self._handle is not None and self._handle.n_devices > 1:
                raise ValueError("execute_fields with valid: this object's handle spans a device group of %d devices; fields with gaps "
                                 "are kriged on one device" % self._handle.n_devices)
        if n_closest_points is not None and int(n_closest_points) > v.shape[0]:
            raise ValueError("n_closest_points exceeds the number of stations")  # what mik_predict_moving_window answers execute()
        P = self._prepare(style, axes, mask, **prepare_kw)
        if n_closest_points is None:
            h = self._upload_and_factor()
        else:  # _solve_moving_window's set-up: no factor
            h = self._get_handle()
            self._set_problem(h)
        self._max_points = max(self._max_points, int(np.prod(P.shape)))
        self._max_fields = max(self._max_fields, v.shape[1])
        P.load(h, self._ndim, with_extra=n_closest_points is None)
        h.set_fields(v.T)
        try:
            if gaps is not None:
                if h.n_devices > 1:
                    raise ValueError("execute_fields with valid: this object's handle spans a device group of %d devices; fields with "
                                     "gaps are kriged on one device" % h.n_devices)
                h.set_field_gaps(gaps.T)
            if n_closest_points is None:
                h.predict()
            else:
                with _singular_as(backend):
                    h.predict_moving_window(int(n_closest_points))
            self.last_timing = h.timing()
            zf = h.get_field_results()  # (before get_results: that one may take the landing zone over)
            ssf = None if gaps is None else h.get_field_sigmasq()
            _, ss = h.get_results()
        finally:
            h.set_fields(None)  # (clears the gaps with the fields)
        if ssf is not None:
            zf, _ = self._finish_fields(zf, ss, style, P.shape, P.mask, backend)
            ssf, _ = self._finish_fields(ssf, ss, style, P.shape, P.mask, backend)
            return zf, ssf
        return self._finish_fields(zf, ss, style, P.shape, P.mask, backend)

    def _finish_fields(self, zf, ss, style, shape, mask, backend):
        """_finish for the (F, npt) planes of execute_fields: the mask is repeated over the field axis."""
        _, ss = self._finish(zf[0], ss, style, shape, mask, backend)
        nf = zf.shape[0]
        if style == "masked":
            zf = np.ma.array(zf, mask=np.broadcast_to(mask, zf.shape).copy())
        elif backend == "vectorized" and zf.size:
            zf = np.ma.array(zf, mask=np.zeros(zf.shape, dtype=bool))
        return zf.reshape((nf,) + tuple(shape)), ss

    # ---------------------------------------------------------------- what execute_cov and execute_block share
    def _grid_or_points(self, style, backend, masked_message):
        if style == "masked":
            raise ValueError(masked_message)
        if style != "grid" and style != "points":
            raise ValueError("style argument must be 'grid' or 'points'")
        self._check_backend(backend, None)

    def _refuse_custom_and_pinv(self, name, custom_why, pinv_why):
        if self.variogram_model == "custom":
            raise NotImplementedError("%s: variogram_model='custom' is evaluated on the host; %s" % (name, custom_why))
        if pinv_why is not None and self.pseudo_inv:  # (None: the call uses no inverse)
            raise ValueError("%s needs a regular inverse: %s for pseudo_inv=True" % (name, pinv_why))

    @staticmethod
    def _refuse_group(h, name, one_device):
        if h is not None and h.n_devices > 1:
            raise ValueError("%s: this object's handle spans a device group of %d devices; %s" % (name, h.n_devices, one_device))

    # ---------------------------------------------------------------- anisotropy tools (libmikvario.so, variography.py)
    def _variography_stations(self, name):
        """The raw station coordinates and values of a 2-D euclidean object -- before the anisotropy adjustment, which is what the tool is
        there to find.  Every refusal is raised before libmikvario.so is loaded."""
        if self._ndim == 3:
            raise ValueError("%s: directions in 3-D need an azimuth and a dip; only the 2-D classes have this tool (the 3-D classes have "
                             "%s_3d)" % (name, name))
        if getattr(self, "coordinates_type", "euclidean") == "geographic":
            raise ValueError("%s: coordinates_type='geographic' is not built; directions and lag vectors are planar" % name)
        self._refuse_group(self._handle, name, "the pairs are binned on one device")
        return self.X_ORIG, self.Y_ORIG, self._values()

    def directional_variogram(self, azimuths, tolerance=22.5, nlags=6, maxlag=None, edges=None, bandwidth=None):
        """Directional experimental semivariograms of this object's stations and values, in the caller's coordinates -- BEFORE the anisotropy
        adjustment: ``lags, semivariance, counts = obj.directional_variogram(azimuths, tolerance=22.5, nlags=6, maxlag=None, edges=None,
        bandwidth=None)``, each (A, nlags).  azimuths in degrees counter-clockwise from +x, the convention of ``anisotropy_angle``.  The
        arguments and results are ``pykrige_amd.variography.directional_variogram``'s.  The 3-D classes, coordinates_type='geographic' and
        a handle that spans a device group raise ``ValueError``."""
        from . import variography

        x, y, v = self._variography_stations("directional_variogram")
        return variography.directional_variogram(x, y, v, azimuths, tolerance=tolerance, nlags=nlags, maxlag=maxlag, edges=edges,
                                                 bandwidth=bandwidth)

    def variogram_map(self, nx, ny, dx, dy):
        """Variogram map of this object's stations and values, in the caller's coordinates -- BEFORE the anisotropy adjustment:
        ``semivariance, counts = obj.variogram_map(nx, ny, dx, dy)``, each (2 ny + 1, 2 nx + 1), cells of dx x dy centred on lag zero.
        The arguments and results are ``pykrige_amd.variography.variogram_map``'s.  The 3-D classes, coordinates_type='geographic' and a
        handle that spans a device group raise ``ValueError``."""
        from . import variography

        x, y, v = self._variography_stations("variogram_map")
        return variography.variogram_map(x, y, v, nx, ny, dx, dy)

    # ---------------------------------------------------------------- the same tools for the 3-D classes (libmikvario3.so, variography3d.py)
    def _variography3d_stations(self, name):
        """The raw station coordinates and values of a 3-D object -- before the anisotropy adjustment.  Every refusal is raised before
        libmikvario3.so is loaded."""
        if self._ndim != 3:
            raise ValueError("%s: this is a 2-D object; the 2-D classes have %s (azimuths only)" % (name, name[:-3]))
        self._refuse_group(self._handle, name, "the pairs are binned on one device")
        return self.X_ORIG, self.Y_ORIG, self.Z_ORIG, self._values()

    def directional_variogram_3d(self, azimuths=None, dips=None, directions=None, tolerance=22.5, nlags=6, maxlag=None, edges=None,
                                 bandwidth=None):
        """Directional experimental semivariograms of this 3-D object's stations and values, in the caller's coordinates -- BEFORE the
        anisotropy adjustment: ``lags, semivariance, counts = obj.directional_variogram_3d(azimuths=None, dips=None, directions=None,
        tolerance=22.5, nlags=6, maxlag=None, edges=None, bandwidth=None)``, each (A, nlags).  Give azimuths and dips in degrees (azimuth
        counter-clockwise from +x, dip upward toward +z) or directions, (A, 3) vectors; ``directions=core.anisotropy_axes([angle_x, angle_y,
        angle_z])`` looks along the principal axes of a candidate rotation.  The arguments and results are
        ``pykrige_amd.variography3d.directional_variogram_3d``'s.  A 2-D object (use ``directional_variogram``) and a handle that spans a
        device group raise ``ValueError``."""
        from . import variography3d

        x, y, z, v = self._variography3d_stations("directional_variogram_3d")
        return variography3d.directional_variogram_3d(x, y, z, v, azimuths=azimuths, dips=dips, directions=directions, tolerance=tolerance,
                                                      nlags=nlags, maxlag=maxlag, edges=edges, bandwidth=bandwidth)

    def variogram_map_3d(self, nx, ny, nz, dx, dy, dz):
        """3-D variogram map of this 3-D object's stations and values, in the caller's coordinates -- BEFORE the anisotropy adjustment:
        ``semivariance, counts = obj.variogram_map_3d(nx, ny, nz, dx, dy, dz)``, each (2 nz + 1, 2 ny + 1, 2 nx + 1), cells of dx x dy x dz
        centred on lag zero.  The arguments and results are ``pykrige_amd.variography3d.variogram_map_3d``'s.  A 2-D object (use
        ``variogram_map``) and a handle that spans a device group raise ``ValueError``."""
        from . import variography3d

        x, y, z, v = self._variography3d_stations("variogram_map_3d")
        return variography3d.variogram_map_3d(x, y, z, v, nx, ny, nz, dx, dy, dz)

    # ---------------------------------------------------------------- the likelihood of the variogram (libmiklik.so, likelihood.py)
    def _likelihood_problem(self, name, anisotropy):
        """(coordinate columns, values, drift, anisotropy keywords) of this object for likelihood.py.  Every refusal is raised before
        libmiklik.so is loaded."""
        from . import likelihood

        if getattr(self, "coordinates_type", "euclidean") == "geographic":
            raise ValueError("%s: coordinates_type='geographic' is not built; the covariance is a function of the Euclidean distance" % name)
        self._refuse_group(self._handle, name, "the covariance matrix is factored on one device")
        likelihood._check_model(name, self.variogram_model)
        drift = None
        if self._universal:
            others = [t for t in ("external_Z_drift", "point_log_drift", "specified_drift", "functional_drift") if getattr(self, t, False)]
            if others:
                raise NotImplementedError("%s: regional_linear is the only drift term whose trend is built (X = [1, x, y(, z)] of the "
                                          "adjusted coordinates); this object also has %s" % (name, ", ".join(t[:-6] for t in others)))
            if self._regional_linear():
                drift = "regional_linear"
        own = likelihood._ANIS2 if self._ndim == 2 else likelihood._ANIS3
        unknown = set(anisotropy) - set(own)
        if unknown:
            raise TypeError("%s: unexpected argument %s (the anisotropy overrides of this class are %s)"
                            % (name, ", ".join(sorted(unknown)), ", ".join(own)))
        anis = {k: getattr(self, k) for k in own}
        anis.update({k: v for k, v in anisotropy.items() if v is not None})
        cols = [self.X_ORIG, self.Y_ORIG] + ([self.Z_ORIG] if self._ndim == 3 else [])
        return cols, self._values(), drift, anis

    def _list_parameters(self):
        psill, rng, nugget = (float(v) for v in self.variogram_model_parameters)
        return [psill + nugget, rng, nugget]

    def neg_log_likelihood(self, variogram_parameters=None, reml=True, **anisotropy):
        """The negative Gaussian log-likelihood of this object's stations and values under its variogram model, one Cholesky factorisation
        on the GPU: ``nll = obj.neg_log_likelihood(variogram_parameters=None, reml=True, **anisotropy)``.  variogram_parameters=None takes
        the object's current parameters, otherwise the constructor's forms (a list with the FULL sill, or a dict).  The anisotropy is the
        object's unless overridden by the constructor's keywords (``anisotropy_scaling``, ``anisotropy_angle``; 3-D:
        ``anisotropy_scaling_y``, ``anisotropy_scaling_z``, ``anisotropy_angle_x``, ``anisotropy_angle_y``, ``anisotropy_angle_z``).  The
        mean is constant; on the universal classes with ``regional_linear`` the trend is X = [1, x, y(, z)] of the adjusted coordinates,
        and any other drift term raises ``NotImplementedError``.  reml=True is the restricted likelihood, False the full one; the formulas
        are ``pykrige_amd.likelihood.neg_log_likelihood``'s.  A matrix that is not positive definite gives ``inf``.  'linear', 'power'
        (ValueError) and 'custom' (NotImplementedError) models, coordinates_type='geographic' and a handle that spans a device group
        (ValueError) are refused before anything is loaded."""
        from . import likelihood

        cols, v, drift, anis = self._likelihood_problem("neg_log_likelihood", anisotropy)
        par = self._list_parameters() if variogram_parameters is None else variogram_parameters
        return likelihood.neg_log_likelihood(*cols, v, self.variogram_model, par, drift=drift, reml=reml, **anis)

    def neg_log_likelihood_grad(self, variogram_parameters=None, reml=True, **anisotropy):
        """``nll, grad = obj.neg_log_likelihood_grad(variogram_parameters=None, reml=True, **anisotropy)``: what ``neg_log_likelihood``
        returns, bit for bit, and its analytic gradient from the same elimination on the GPU (libmikgrad.so).  grad is in natural units
        in the order of ``pykrige_amd.likelihood.GRAD_NAMES_2D`` / ``GRAD_NAMES_3D``: psill (the partial sill, the nugget held), range,
        nugget, then this class's anisotropy keywords, angles per degree.  The arguments, the trend (``regional_linear`` on the
        universal classes; the gradient with the trend columns held is exact, see ``likelihood.neg_log_likelihood_grad``) and the
        refusals are ``neg_log_likelihood``'s: 'linear', 'power' (ValueError) and 'custom' (NotImplementedError) models,
        coordinates_type='geographic' and a handle that spans a device group (ValueError), any other drift term
        (``NotImplementedError``).  A matrix that is not positive definite gives ``inf`` and a gradient of NaN."""
        from . import likelihood

        cols, v, drift, anis = self._likelihood_problem("neg_log_likelihood_grad", anisotropy)
        par = self._list_parameters() if variogram_parameters is None else variogram_parameters
        return likelihood.neg_log_likelihood_grad(*cols, v, self.variogram_model, par, drift=drift, reml=reml, **anis)

    def fit_variogram_ml(self, start=None, fit_anisotropy=False, reml=True, bounds=None, **anisotropy):
        """Maximum-likelihood / REML fit of this object's variogram model (and, with fit_anisotropy, of its anisotropy) to its stations
        and values -- binning-free: ``fit = obj.fit_variogram_ml(start=None, fit_anisotropy=False, reml=True, bounds=None, **anisotropy)``.
        start=None begins at the object's current parameters and anisotropy (the constructor's least-squares fit, unless parameters were
        given).  Returns ``pykrige_amd.likelihood.MLFit``: ``fit.variogram_parameters`` in the constructor's list form and
        ``fit.anisotropy`` as the constructor's keywords, ``fit.nll``, ``fit.n_evaluations``, ``fit.success``; the object itself is not
        changed -- hand the fit to ``update_variogram_model`` or to a new object.  The trend and the refusals are those of
        ``neg_log_likelihood``: 'linear', 'power' and 'custom' models, coordinates_type='geographic', a device group, and on the universal
        classes any drift term but ``regional_linear`` (``NotImplementedError``).  ``method='l-bfgs-b'``, given by keyword, is passed
        on: the quasi-Newton search with the analytic gradient (``likelihood.fit_variogram_ml``); the default is 'nelder-mead'."""
        from . import likelihood

        anisotropy = dict(anisotropy)
        method = anisotropy.pop("method", "nelder-mead")
        cols, v, drift, anis = self._likelihood_problem("fit_variogram_ml", anisotropy)
        return likelihood.fit_variogram_ml(*cols, v, self.variogram_model, start=self._list_parameters() if start is None else start,
                                           fit_anisotropy=fit_anisotropy, drift=drift, reml=reml, bounds=bounds, method=method, **anis)

    # ---------------------------------------------------------------- Vecchia's approximation of it (libmikvecchia.so, vecchia.py)
    def neg_log_likelihood_vecchia(self, variogram_parameters=None, m=30, order="random", seed=0, plan=None, reml=True, **anisotropy):
        """``neg_log_likelihood`` in Vecchia's approximation, for station sets past the N x N matrix:
        ``nll = obj.neg_log_likelihood_vecchia(variogram_parameters=None, m=30, order="random", seed=0, plan=None, reml=True,
        **anisotropy)``.  Every station is conditioned on its m nearest predecessors in the order (``pykrige_amd.vecchia.VecchiaPlan``);
        with m >= N - 1 the value is the exact likelihood.  plan: a ``VecchiaPlan`` of this object's adjusted stations to reuse, else one
        is built and dropped.  The parameters, the anisotropy overrides, the trend (``regional_linear`` on the universal classes) and the
        refusals are ``neg_log_likelihood``'s: 'linear', 'power' (ValueError) and 'custom' (NotImplementedError) models,
        coordinates_type='geographic' and a handle that spans a device group (ValueError), any other drift term
        (``NotImplementedError``) -- all before anything is loaded."""
        from . import vecchia

        cols, v, drift, anis = self._likelihood_problem("neg_log_likelihood_vecchia", anisotropy)
        par = self._list_parameters() if variogram_parameters is None else variogram_parameters
        return vecchia.neg_log_likelihood_vecchia(*cols, v, self.variogram_model, par, m=m, order=order, seed=seed, plan=plan, drift=drift,
                                                  reml=reml, **anis)

    def fit_variogram_vecchia(self, m=30, order="random", seed=0, start=None, fit_anisotropy=False, reml=True, bounds=None, **anisotropy):
        """``fit_variogram_ml`` on Vecchia's objective: ``fit = obj.fit_variogram_vecchia(m=30, order="random", seed=0, start=None,
        fit_anisotropy=False, reml=True, bounds=None, **anisotropy)``.  One ``VecchiaPlan`` built in the start metric serves the whole
        Nelder-Mead search (``pykrige_amd.vecchia.fit_variogram_vecchia``); there is no gradient method.  start=None begins at the
        object's current parameters and anisotropy.  Returns ``pykrige_amd.likelihood.MLFit``; the object itself is not changed.  The
        trend (``regional_linear``) and the refusals are those of ``neg_log_likelihood``: 'linear', 'power' and 'custom' models,
        coordinates_type='geographic', a device group, and any other drift term (``NotImplementedError``)."""
        from . import vecchia

        cols, v, drift, anis = self._likelihood_problem("fit_variogram_vecchia", anisotropy)
        return vecchia.fit_variogram_vecchia(*cols, v, self.variogram_model, m=m, order=order, seed=seed,
                                             start=self._list_parameters() if start is None else start, fit_anisotropy=fit_anisotropy,
                                             drift=drift, reml=reml, bounds=bounds, **anis)

    # ---------------------------------------------------------------- ... with its analytic gradient (libmikvgrad.so, vecchia_grad.py)
    def neg_log_likelihood_vecchia_grad(self, variogram_parameters=None, m=30, order="random", seed=0, plan=None, reml=True, **anisotropy):
        """``nll, grad = obj.neg_log_likelihood_vecchia_grad(variogram_parameters=None, m=30, order="random", seed=0, plan=None,
        reml=True, **anisotropy)``: what ``neg_log_likelihood_vecchia`` returns, bit for bit, and its analytic gradient from the same
        local factorisations on the GPU (``pykrige_amd.vecchia_grad.neg_log_likelihood_vecchia_grad``).  grad is in natural units in the
        order of ``pykrige_amd.likelihood.GRAD_NAMES_2D`` / ``GRAD_NAMES_3D``: psill (the partial sill, the nugget held), range, nugget,
        then this class's anisotropy keywords, angles per degree.  plan: a ``VecchiaGradPlan`` of this object's adjusted stations to
        reuse, else one is built and dropped.  The parameters, the anisotropy overrides, the trend (``regional_linear`` on the universal
        classes) and the refusals are ``neg_log_likelihood``'s: 'linear', 'power' (ValueError) and 'custom' (NotImplementedError)
        models, coordinates_type='geographic' and a handle that spans a device group (ValueError), any other drift term
        (``NotImplementedError``) -- all before anything is loaded."""
        from . import vecchia_grad

        cols, v, drift, anis = self._likelihood_problem("neg_log_likelihood_vecchia_grad", anisotropy)
        par = self._list_parameters() if variogram_parameters is None else variogram_parameters
        return vecchia_grad.neg_log_likelihood_vecchia_grad(*cols, v, self.variogram_model, par, m=m, order=order, seed=seed, plan=plan,
                                                            drift=drift, reml=reml, **anis)

    def fit_variogram_vecchia_grad(self, m=30, order="random", seed=0, start=None, fit_anisotropy=False, reml=True, bounds=None,
                                   **anisotropy):
        """``fit_variogram_vecchia`` by a quasi-Newton search: ``fit = obj.fit_variogram_vecchia_grad(m=30, order="random", seed=0,
        start=None, fit_anisotropy=False, reml=True, bounds=None, **anisotropy)``.  One ``VecchiaGradPlan`` built in the start metric
        serves the whole L-BFGS-B search on the analytic gradient (``pykrige_amd.vecchia_grad.fit_variogram_vecchia_grad``), with the
        Nelder-Mead finish of ``fit_variogram_ml(method='l-bfgs-b')``.  start=None begins at the object's current parameters and
        anisotropy.  Returns ``pykrige_amd.likelihood.MLFit``; the object itself is not changed.  The trend (``regional_linear``) and
        the refusals are those of ``neg_log_likelihood``: 'linear', 'power' and 'custom' models, coordinates_type='geographic', a
        device group, and any other drift term (``NotImplementedError``)."""
        from . import vecchia_grad

        cols, v, drift, anis = self._likelihood_problem("fit_variogram_vecchia_grad", anisotropy)
        return vecchia_grad.fit_variogram_vecchia_grad(*cols, v, self.variogram_model, m=m, order=order, seed=seed,
                                                       start=self._list_parameters() if start is None else start,
                                                       fit_anisotropy=fit_anisotropy, drift=drift, reml=reml, bounds=bounds, **anis)

    def _resident_problem(self, P, name, one_device):
        """The handle with this object's problem set (only if its key changed) and the points P loaded: (handle, factor key).
        _upload_and_factor without its factor(): mik_predict_cov / mik_predict_block refuse (an oversized P among the reasons) before
        they launch anything and factor themselves if no factor is resident."""
        h = self._get_handle()
        self._refuse_group(h, name, one_device)
        key = self._factor_key_for(h)
        self.factor_reused = key is not None and key == getattr(self, "_factor_key", None)
        if not self.factor_reused:
            self._set_problem(h)
        self._max_points = max(self._max_points, P.npt)
        P.load(h, self._ndim)
        return h, key

    # ---------------------------------------------------------------- error covariance between prediction points (mik_predict_cov)
    _COV_DOC = """Kriged values and the kriging error covariance between the prediction points.

        ``zvalues, cov = obj.execute_cov(style, xpoints, ypoints[, zpoints], backend="vectorized", specified_drift_arrays=None)``

        ``style`` is ``'points'`` or ``'grid'``.  ``zvalues`` is what ``execute()`` returns first for the same call (same shape, type and
        bits).  ``cov`` is a C-contiguous float64 ndarray of shape ``(P, P)``, ``P = prod(zvalues.shape)``, in the flattened order of
        ``zvalues``; it is exactly symmetric and ``diag(cov)`` is ``execute()``'s ``sigmasq`` bit for bit.  It is what the standard error of
        an areal mean, a total or a difference needs (``w @ cov @ w``) and what conditional realisations are drawn from; scikit-learn calls
        it ``predict(return_cov=True)``.

        The identity.  For points p, q let ``b(.)`` be the right-hand sides exactly as ``execute()`` forms them (drift rows, the border
        row and the ``exact_values`` zeroing included) and ``e_p = Z(p) - zhat(p)``.  Then
        ``cov(e_p, e_q) = -gamma*(d_pq) - b(p)^T A^-1 b(q)`` with ``gamma*(d) = 0 if d <= eps`` (the library's exact-hit eps) and the
        object's variogram at ``d`` otherwise; ``d_pq`` is the distance between the adjusted points (geographic coordinates: the
        great-circle distance).  It holds for ordinary and universal kriging alike; ``p = q`` is ``sigmasq = -b^T A^-1 b``, and with
        ``exact_values=True`` the rows of points that sit on a station are zero.  Everything comes from the one resident inverse: two
        matrix products on the device, ``2 P M^2 + P^2 M`` flop for a kriging matrix of order M, and ``P^2`` doubles copied back.

        ``specified_drift_arrays`` is the universal-kriging classes' argument of ``execute()``; the ordinary classes accept only
        ``None``.  There is no ``n_closest_points``: the windows of a moving window differ from point to point, so no joint covariance
        exists.  ``style='masked'`` raises ``ValueError`` (set the unmasked points as ``'points'``), any other unknown style and an
        empty point list raise ``ValueError``, ``variogram_model='custom'`` raises ``NotImplementedError`` (the callable runs on the
        host), ``pseudo_inv=True`` raises ``ValueError`` (the identity needs a regular inverse), a handle that spans a device group
        raises ``ValueError``, and a ``P`` whose device buffers (two of ``P x M`` and one of ``P x P`` doubles, rounded up to 128) would
        exceed a quarter of device memory raises ``ValueError`` naming the largest ``P`` that fits.  ``execute()`` and
        ``execute_fields()`` are untouched: a call after ``execute_cov`` returns the bits it returned before."""

    def _execute_cov(self, style, axes, backend, specified_drift_arrays, universal):
        """execute_cov of the four classes: every argument is checked on the host before the device is touched."""
        self._grid_or_points(style, backend, "execute_cov: style 'masked' has no covariance matrix; pass the unmasked points as style 'points'")
        if not universal and specified_drift_arrays is not None:
            raise ValueError("execute_cov: specified_drift_arrays belongs to the universal-kriging classes")
        self._refuse_custom_and_pinv("execute_cov", "the covariance between points is not built for it", "the covariance identity does not hold")
        self._refuse_group(self._handle, "execute_cov", "the covariance is computed on one device")
        P = self._prepare(style, axes, None, **(dict(specified_drift_arrays=specified_drift_arrays, backend=backend) if universal else {}))
        if P.npt == 0:
            raise ValueError("execute_cov: no points")
        h, key = self._resident_problem(P, "execute_cov", "the covariance is computed on one device")
        cov = h.predict_cov()
        self._factor_key = key
        self.last_timing = h.timing()
        z, ss = h.get_results()
        z, _ = self._finish(z, ss, style, P.shape, None, backend)
        return z, cov

    # ---------------------------------------------------------------- block kriging of cell averages (mik_predict_block)
    _BLOCK_DOC = """Block kriging: the kriged average over a block around every point, and its error variance.

        ``zvalues, sigmasq = obj.execute_block(style, xpoints, ypoints[, zpoints], block_size, n_disc=4, backend="vectorized")``

        ``style`` is ``'grid'`` or ``'points'``; the points are the block CENTRES, and ``zvalues`` and ``sigmasq`` have the shape and
        type ``execute()`` returns for the same call.  ``block_size`` is a positive scalar or one value per axis: the block's edge
        lengths in the caller's raw coordinates.  ``n_disc`` is a positive int or one per axis: the block is discretised into
        ``nd = prod(n_disc)`` nodes, ``nd <= 512``, cell-centred and regular as GSLIB's ``kt3d`` places them (``nxdis``, ``nydis``,
        ``nzdis``): along an axis of length ``L`` with ``n`` nodes the offsets from the centre are ``((i + 0.5) / n - 0.5) L``; node
        order is x fastest, then y, then z.  The anisotropy adjustment is linear, so an adjusted node is the adjusted centre plus
        ``T u`` with ``T = stretch . rot``: the ``nd`` adjusted offsets are formed once per call, and the centres take the path of
        ``execute()``.

        The definition.  With ``b(.)`` the right-hand side exactly as ``execute()`` forms it at a node (the ``exact_values`` zeroing
        where a node is within ``eps`` of a station, drift rows and the border row included),
        ``bbar = (sum_u b(node_u)) / nd`` (summed in node order, one division), ``z_V = c . bbar`` and
        ``sigma^2_V = -gbar - bbar^T A^-1 bbar`` with ``gbar = (sum_u sum_v gamma*(|T (u - v)|)) / nd^2``, ``gamma*(d) = 0 if d <= eps``
        and the object's variogram otherwise.  This is exactly the estimate, and the error variance, of the ARITHMETIC MEAN of ``Z``
        over the block's ``nd`` nodes: the same quantity as the mean of the matching ``nd x nd`` block of ``execute_cov``'s matrix on
        the nodes (and ``zvalues`` is the mean of its ``z``), without that matrix and at one contraction per block instead of one per
        node.  A nugget is therefore treated as variation of ``Z`` itself: it averages down with ``nd`` (it is not measurement
        error that a block average would be free of).  ``n_disc=1`` is ``execute()`` at the centres.

        Drift terms: ``regional_linear`` takes the mean of the node coordinates and ``point_log`` the mean of the well term at the
        nodes, both on the device; ``functional`` drift callables are evaluated on the host at the adjusted nodes and averaged in node
        order.  ``external_Z`` and ``specified`` drifts raise ``NotImplementedError``.  ``style='masked'`` and any unknown style
        raise ``ValueError``; a non-positive or wrong-length ``block_size`` or ``n_disc`` and ``nd > 512`` raise ``ValueError``;
        ``coordinates_type='geographic'`` raises ``ValueError`` (the blocks of a lon / lat grid are not congruent);
        ``pseudo_inv=True`` raises ``ValueError``; a handle that spans a device group raises ``ValueError``;
        ``variogram_model='custom'`` raises ``NotImplementedError``.  ``n_closest_points`` is not an argument of this call: blocks
        kriged through the moving window have a call of their own, ``execute_block_window()``.  ``execute()``,
        ``execute_fields()``, ``execute_cov()`` and ``cross_validate()`` are untouched: a call after ``execute_block`` returns the bits
        it returned before."""

    def _execute_block(self, style, axes, block_size, n_disc, backend):
        """execute_block of the four classes: every argument is checked on the host before the device is touched."""
        self._grid_or_points(style, backend, "execute_block: style 'masked' is not built; pass the unmasked block centres as style 'points'")
        off = core.block_node_offsets(self._ndim, block_size, n_disc)
        if getattr(self, "coordinates_type", "euclidean") == "geographic":
            raise ValueError("execute_block: coordinates_type='geographic' is not built (the blocks of a lon / lat grid are not congruent)")
        self._refuse_custom_and_pinv("execute_block", "block kriging is not built for it", "the block variance is not defined")
        if getattr(self, "external_Z_drift", False) or getattr(self, "specified_drift", False):
            raise NotImplementedError("execute_block: external_Z and specified drifts are given point by point; their block averages are not built")
        self._refuse_group(self._handle, "execute_block", "blocks are kriged on one device")
        off = core.adjust_offsets(off, self._ndim, self._scaling(), self._angle())
        P = self._prepare(style, axes, None)
        if getattr(self, "functional_drift", False) and P.npt:
            # the callables at the adjusted nodes (centre + T u), averaged in node order: the points' extra_rows, already averaged
            ctr = np.asarray(P.arrays, dtype=np.float64)
            rows = []
            for f in self.functional_drift_terms:
                acc = None
                for u in off:
                    v = np.asarray(f(*[ctr[:, k] + u[k] for k in range(self._ndim)]), dtype=np.float64)
                    acc = v if acc is None else acc + v
                rows.append(acc / float(off.shape[0]))
            P.extra = np.array(rows, dtype=np.float64)
        h, key = self._resident_problem(P, "execute_block", "blocks are kriged on one device")
        h.predict_block(off)
        self._factor_key = key
        self.last_timing = h.timing()
        z, ss = h.get_results()
        return self._finish(z, ss, style, P.shape, None, backend)

    # ---------------------------------------------------------------- block kriging through the moving window (mik_predict_block_window)
    _BLOCK_WINDOW_DOC = """Block kriging through the moving window: every block kriged from the k stations nearest to its centre.

        ``zvalues, sigmasq = obj.execute_block_window(style, xpoints, ypoints[, zpoints], block_size, n_closest_points, n_disc=4,
        backend="loop")``

        ``style``, the points (the block CENTRES), ``block_size``, ``n_disc``, the ``nd = prod(n_disc) <= 512`` cell-centred nodes, their
        order and their adjusted offsets ``T u`` are ``execute_block()``'s; ``n_closest_points`` and ``backend`` follow the moving window of
        ``execute()``.  No kriging matrix of all stations is formed or inverted, so the call serves station sets that have no N x N
        inverse, and ``pseudo_inv`` plays no part.

        The definition.  The window of a block is chosen by the centre: the k stations nearest to the adjusted centre ``p``, ascending by
        (squared distance, station index) -- exactly the set and order ``execute(..., n_closest_points=k)`` selects at ``p``; the nodes do
        not take part in the choice.  With ``s_j`` the selected stations,
        ``bbar_j = (sum_u g(|p + T u - s_j|)) / nd`` (summed in node order, one division) with ``g(d) = 0 if exact_values and d <= eps,
        else -gamma(d)``, and ``bbar_k = 1``.  The ``(k + 1) x (k + 1)`` local system of the moving window gives the weights ``lam`` and
        the multiplier ``mu`` from ``bbar``; ``z_V = lam . Z_sel`` and ``sigma^2_V = -lam . bbar - mu - gbar`` with ``gbar`` exactly
        ``execute_block()``'s.  This is the estimate, and the error variance, of the ARITHMETIC MEAN of ``Z`` over the block's nodes,
        kriged from the window's stations; a nugget averages down with ``nd`` as in ``execute_block()``.  ``n_disc=1`` is
        ``execute(style, ..., n_closest_points=k)`` bit for bit.

        ``OrdinaryKriging`` and ``OrdinaryKriging3D`` take ``backend='loop'`` (and ``'C'`` in 2-D; all run the same device path); the
        universal-kriging classes have no moving window and raise ``ValueError``.  ``style='masked'`` and any unknown style raise
        ``ValueError``; a non-positive or wrong-length ``block_size`` or ``n_disc`` and ``nd > 512`` raise ``ValueError``;
        ``n_closest_points <= 1`` and ``n_closest_points > N`` raise ``ValueError``; ``coordinates_type='geographic'`` raises
        ``ValueError``; a handle that spans a device group raises ``ValueError``; ``variogram_model='custom'`` raises
        ``NotImplementedError``.  A singular local system raises as in ``execute()`` (``ValueError('Singular matrix')`` for backend
        'C').  ``last_timing`` is set.  A factor that ``execute()`` left on the device is neither used nor lost, and ``execute()``,
        ``execute_block()`` and the other calls return after this one the bits they returned before."""

    def _execute_block_window(self, style, axes, block_size, n_closest_points, n_disc, backend):
        """execute_block_window of the four classes: every argument is checked on the host before the device is touched."""
        if style == "masked":
            raise ValueError("execute_block_window: style 'masked' is not built; pass the unmasked block centres as style 'points'")
        if style != "grid" and style != "points":
            raise ValueError("style argument must be 'grid' or 'points'")
        if n_closest_points is None:
            raise ValueError("execute_block_window needs n_closest_points (the global form is execute_block())")
        self._check_backend(backend, n_closest_points)
        off = core.block_node_offsets(self._ndim, block_size, n_disc)
        if getattr(self, "coordinates_type", "euclidean") == "geographic":
            raise ValueError("execute_block_window: coordinates_type='geographic' is not built (the blocks of a lon / lat grid are not congruent)")
        self._refuse_custom_and_pinv("execute_block_window", "block kriging is not built for it", None)
        self._refuse_group(self._handle, "execute_block_window", "blocks are kriged on one device")
        k = int(n_closest_points)
        if k > int(np.size(self._values())):
            raise ValueError("n_closest_points exceeds the number of stations")  # what mik_predict_moving_window answers execute()
        off = core.adjust_offsets(off, self._ndim, self._scaling(), self._angle())
        P = self._prepare(style, axes, None)
        h = self._get_handle()
        self._refuse_group(h, "execute_block_window", "blocks are kriged on one device")
        key = self._factor_key_for(h)
        if key is None or key != getattr(self, "_factor_key", None):  # (a factored problem on the handle is this object's: it stays, with its factor)
            self._set_problem(h)
        self._max_points = max(self._max_points, P.npt)
        P.load(h, self._ndim, with_extra=False)
        with _singular_as(backend):
            h.predict_block_window(off, k)
        self.last_timing = h.timing()
        z, ss = h.get_results()
        return self._finish(z, ss, style, P.shape, None, backend)

    # ---------------------------------------------------------------- fields with gaps through the moving window (mik_predict_window_gaps)
    _FIELDS_WINDOW_DOC = """Krige F value fields with missing stations through the moving window.

        ``zvalues, sigmasq = obj.execute_fields_window(style, xpoints, ypoints[, zpoints], values, n_closest_points, valid=None,
        backend="loop")``

        ``values`` is ``(N, F)`` or ``(N,)`` (F = 1) as in ``execute_fields()``.  ``valid`` is a boolean array of the shape of ``values``
        and True means "measured"; it follows the rules of ``execute_fields()``'s ``valid``: boolean dtype only, entries of ``values``
        where it is False are ignored (they may be NaN or inf and are never read), entries where it is True must be finite.
        ``style`` is ``'points'`` or ``'grid'``.  Both outputs are plain float64 arrays of shape ``(F,) + shape``, ``shape`` being what
        ``execute()`` returns for the same points: every field has its own sigma^2.

        ``zvalues[f]`` and ``sigmasq[f]`` are what an object built from the stations with ``valid[:, f]`` alone returns from
        ``execute(style, ..., n_closest_points=k)`` -- an object with this object's variogram parameters, anisotropy, centre,
        ``exact_values`` and adjusted coordinates.  The window of a point is its k nearest stations among those field f has, ascending
        by (distance, station index in the order the stations were given in).  No kriging matrix of all stations is formed or inverted:
        the call serves station sets that have no N x N inverse, and ``pseudo_inv`` plays no part.

        Fields with the same ``valid`` column form a pattern.  A pattern shares one neighbour search, one set of right-hand sides and one
        sigma^2 (its fields share the bits of their ``sigmasq`` planes); its fields go through the local solver in row groups, up to
        G - 2 per pass for windows up to 256 as in ``execute_fields(..., n_closest_points=k)``, and plane f is bit for bit the one-field
        call with that column.  P distinct patterns therefore cost about P one-field window calls, one shared pattern about one
        multi-field call.  A pattern without a gap runs the search of ``execute()``: its planes are bit for bit those of
        ``execute_fields(..., n_closest_points=k)``; ``valid=None`` makes every field such a pattern.

        ``n_closest_points`` and ``backend`` follow the moving window of ``execute()``: ``OrdinaryKriging`` and ``OrdinaryKriging3D``
        take ``backend='loop'`` (and ``'C'`` in 2-D; all run the same device path); the universal-kriging classes have no moving window
        and raise ``ValueError``.  ``style='masked'`` and any unknown style raise ``ValueError``; ``n_closest_points <= 1`` raises
        ``ValueError``; a field with fewer than ``n_closest_points`` valid stations raises ``ValueError`` naming the first such field; a
        window beyond the device's neighbour search in on-chip memory (more than 7936 stations by default) raises ``ValueError``; a
        handle that spans a device group raises ``ValueError``; ``variogram_model='custom'`` raises ``NotImplementedError``.  A singular
        local system raises as in ``execute()``.  ``last_timing`` is set, its times summed over the patterns.

        No factor is needed, built or invalidated: a factor that ``execute()`` left on the device is neither used nor lost.  The points
        are set as by any ``execute()``, and the device planes of an earlier ``execute()`` / ``execute_fields()`` are overwritten (arrays
        those calls returned are the caller's and stay).  ``cross_validate_window()`` keeps its results in buffers of its own, and so do
        ``cross_validate()``, ``execute_cov()`` and the gap planes of ``execute_fields(..., valid=)``, which every such call writes anew:
        all of them return after this call the bits they returned before.  ``execute_fields(..., n_closest_points=, valid=)`` still
        raises ``NotImplementedError``: this call is the moving window with gaps."""

    def _execute_fields_window(self, style, axes, values, n_closest_points, valid, backend):
        """execute_fields_window of the four classes: every argument is checked on the host before the device is touched."""
        if style == "masked":
            raise ValueError("execute_fields_window: style 'masked' is not built; pass the unmasked points as style 'points'")
        if style != "grid" and style != "points":
            raise ValueError("style argument must be 'grid' or 'points'")
        if n_closest_points is None:
            raise ValueError("execute_fields_window needs n_closest_points (the global form is execute_fields(..., valid=))")
        self._check_backend(backend, n_closest_points)
        self._refuse_custom_and_pinv("execute_fields_window", "the moving window with gaps is not built for it", None)
        v = self._field_values(values, valid)
        gaps = None if valid is None else self._field_gaps(values, v, valid, zero=False)
        k = int(n_closest_points)
        have = gaps.sum(axis=0) if gaps is not None else np.full(v.shape[1], v.shape[0])
        short = np.flatnonzero(have < k)
        if short.size:
            raise ValueError("execute_fields_window: field %d has %d valid stations, fewer than n_closest_points = %d"
                             % (int(short[0]), int(have[short[0]]), k))
        self._refuse_group(self._handle, "execute_fields_window", "fields with gaps are kriged on one device")
        P = self._prepare(style, axes, None)
        h = self._get_handle()
        self._refuse_group(h, "execute_fields_window", "fields with gaps are kriged on one device")
        key = self._factor_key_for(h)
        if key is None or key != getattr(self, "_factor_key", None):  # (a factored problem on the handle is this object's: it stays, with its factor)
            self._set_problem(h)
        self._max_points = max(self._max_points, P.npt)
        self._max_fields = max(self._max_fields, v.shape[1])
        P.load(h, self._ndim, with_extra=False)
        h.set_fields(v.T)
        try:
            with _singular_as(backend):
                zf, ssf = h.predict_window_gaps(k, None if gaps is None else gaps.T)
            self.last_timing = h.timing()
        finally:
            h.set_fields(None)
        nf = v.shape[1]
        return zf.reshape((nf,) + tuple(P.shape)), ssf.reshape((nf,) + tuple(P.shape))

    # ---------------------------------------------------------------- leave-one-out cross-validation (mik_cross_validate)
    _CV_DOC = """Leave-one-out cross-validation on the device: every station kriged from the other stations.

        ``zhat, sigmasq = obj.cross_validate(values=None, n_closest_points=None, backend="vectorized", folds=None)``

        ``values`` is ``None`` (the object's own values), ``(N,)`` or ``(N, F)`` (F fields measured at the stations, as in
        ``execute_fields``).  ``zhat`` has shape ``(N,)`` for ``None`` or 1-D values and ``(F, N)`` for 2-D values; ``sigmasq`` has
        shape ``(N,)`` and does not depend on the values.  Both are plain float64 ndarrays in the order the stations were given in.
        The residuals are ``values - zhat``.  The variogram, the drift terms, the anisotropy and ``exact_values`` are the object's; the
        variogram is not fitted again without station i.

        Global form (``n_closest_points=None``): entry i is station i kriged from ALL other stations.  The kriging matrix has a zero
        diagonal, so with ``B`` its inverse and ``c = B[:, :N] v`` the block inverse gives ``zhat_i = v_i - c_i / B_ii`` and
        ``sigmasq_i = 1 / B_ii`` exactly, for ordinary and universal kriging alike (drift and border rows included): all N predictions
        of all F fields cost the one factorisation ``execute()`` needs anyway (and reuses), one pass over the inverse and a
        diagonal read.  ``exact_values`` plays no part (no other station lies within eps of station i unless it is a duplicate, and
        duplicated stations make the matrix singular).  ``B_ii`` is used as computed: a zero or non-finite one gives inf / nan in
        that entry and nothing is raised.  An object with ``pseudo_inv=True`` raises ``ValueError``: the identity needs a regular
        inverse.  Runs on the handle's own device; a device group takes no share in it.

        Windowed form (``n_closest_points=k``: station i kriged from its k nearest other stations): not built.  The argument is
        checked by the backend rules of ``execute()`` (the universal-kriging classes raise as for any moving window) and the call then
        raises ``NotImplementedError``; nothing else is computed in its place.  The windowed form has a call of its own,
        ``cross_validate_window(n_closest_points)``.

        Groups (``folds``, a keyword after the three above; ``None`` is the leave-one-out form described so far).  ``folds=K``, an
        integer with ``2 <= K <= N``, makes K contiguous folds in the order the stations were given in, the first ``N % K`` of
        ``N // K + 1`` stations and the rest of ``N // K`` (scikit-learn's ``KFold(K)`` without shuffle).  ``folds=labels``, an integer
        array of shape ``(N,)`` with at least two distinct values, holds out together the stations that carry the same label
        (leave-group-out: spatial blocks, transects, campaigns); the label values themselves do not matter.  For a fold ``S`` and
        ``R`` = everything else (drift and border rows included) the block inverse gives
        ``B_SS^-1 = A_SS - A_SR A_RR^-1 A_RS`` and hence ``zhat_S = v_S - B_SS^-1 c_S`` and ``sigmasq_S = diag(B_SS^-1)``, exactly:
        every fold costs a Cholesky factorisation of its own ``|S| x |S|`` block of the one resident inverse, never another
        factorisation of the kriging matrix.  ``folds=N`` is leave-one-out by this route (within rounding of ``folds=None``, not
        the same bits).  Every fold leaves at least one station; whether the remainder still determines the drift terms is the
        caller's business: a remainder too small or too degenerate for them makes ``B_SS`` ill-conditioned, like a near-zero
        ``B_ii``.  A fold whose block is not numerically positive definite (a non-positive or non-finite pivot) returns NaN in
        ``zhat`` and ``sigmasq`` for its stations; the other folds are unaffected and nothing is raised.  A ``folds`` that is not
        of integer type, has the wrong shape, a ``K`` out of range or fewer than two distinct labels raises ``ValueError``.

        The points and results an earlier ``execute()`` left on the device stay as they are."""

    def _fold_labels(self, folds):
        """folds of cross_validate -> (labels 0 .. nfolds - 1 as int32 (N,), nfolds); every error is a ValueError."""
        n = int(np.size(self._values()))
        if isinstance(folds, (bool, np.bool_)):
            raise ValueError("folds must be an integer K or an integer array of N labels")
        if isinstance(folds, (int, np.integer)):
            k = int(folds)
            if not 2 <= k <= n:
                raise ValueError("folds=%d: the number of folds must lie between 2 and the number of stations (%d)" % (k, n))
            sizes = np.full(k, n // k, dtype=np.int64)
            sizes[:n % k] += 1
            return np.repeat(np.arange(k, dtype=np.int32), sizes), k
        lab = np.asarray(folds)
        if lab.dtype.kind not in "iu":
            raise ValueError("folds must be an integer K or an array of integer labels; got dtype %s" % lab.dtype)
        if lab.shape != (n,):
            raise ValueError("folds has shape %s; the object has %d stations (shape (%d,))" % (lab.shape, n, n))
        uniq, inv = np.unique(lab, return_inverse=True)
        if uniq.size < 2:
            raise ValueError("folds needs at least two distinct labels: one group would leave no station to krige from")
        return np.ascontiguousarray(inv.reshape(n), dtype=np.int32), int(uniq.size)

    def cross_validate(self, values=None, n_closest_points=None, backend="vectorized", folds=None):
        self._check_backend(backend, n_closest_points)
        v = None if values is None else self._field_values(values)
        fold = None if folds is None else self._fold_labels(folds)
        if n_closest_points is not None:
            raise NotImplementedError("cross_validate: the windowed form (n_closest_points) is not built; n_closest_points=None kriges "
                                      "every station from all other stations")
        if self.pseudo_inv:
            raise ValueError("cross_validate needs a regular inverse: the leave-one-out identity does not hold for pseudo_inv=True")
        h = self._upload_and_factor()
        if v is not None:
            self._max_fields = max(self._max_fields, v.shape[1])
            h.set_fields(v.T)
        try:
            zhat, ss = h.cross_validate(0) if fold is None else h.cross_validate_folds(*fold)
        finally:
            if v is not None:
                h.set_fields(None)
        return (zhat if v is not None and np.ndim(values) == 2 else zhat[0]), ss

    cross_validate.__doc__ = _CV_DOC

    # ---------------------------------------------------------------- windowed leave-one-out cross-validation (mik_cross_validate_window)
    def cross_validate_window(self, n_closest_points, values=None, backend="loop"):
        """Windowed leave-one-out cross-validation on the device: every station kriged from its k nearest OTHER stations.

        ``zhat, sigmasq = obj.cross_validate_window(n_closest_points, values=None, backend="loop")``

        The score of the predictor ``execute(..., n_closest_points=k)``: entry i is what an object built from the other N - 1 stations
        returns from ``execute('points', x_i, y_i[, z_i], n_closest_points=k)`` -- an object with this object's variogram parameters,
        centre and adjusted coordinates (the variogram is not fitted again without station i).  The anisotropy, ``exact_values`` and
        the coordinate type are the object's; ``pseudo_inv`` plays no part, as in ``execute()`` with a window.  No kriging matrix of all
        stations is formed or inverted, so the call also serves station sets for which the global form ``cross_validate()`` has no
        N x N inverse; a factor that ``execute()`` left on the device is not used.

        ``values`` and the shapes are ``cross_validate()``'s: ``None`` (the object's own values), ``(N,)`` or ``(N, F)``; ``zhat`` is
        ``(N,)`` for ``None`` or 1-D values and ``(F, N)`` for 2-D values, ``sigmasq`` is ``(N,)`` and does not depend on the values.
        Both are plain float64 ndarrays in the order the stations were given in.  Several fields share the neighbour search, the
        right-hand sides and, for windows up to 256, the factorisation of every local system (as in ``execute_fields``): plane f has
        the bits of the one-field call.

        Station i is left out of its own window by its index, never by its distance: a station coincident with station i stays in the
        window, at distance 0.  With ``exact_values=True`` its value is then the answer and ``sigmasq`` is 0.  Ties in distance are
        broken by station index, as in ``execute()``.

        ``n_closest_points`` and ``backend`` follow the moving window of ``execute()``: ``OrdinaryKriging`` and ``OrdinaryKriging3D``
        take ``backend='loop'`` or ``'C'`` (both run the same device path); the universal-kriging classes have no moving window and
        raise ``ValueError``; ``n_closest_points <= 1`` raises ``ValueError``.  ``n_closest_points > N - 1`` raises ``ValueError``
        (only N - 1 other stations exist), and so does a window beyond the device's neighbour search in on-chip memory (more than
        7936 stations by default): at that window size the global form is the tool.  A singular local system raises as in
        ``execute()`` (``ValueError('Singular matrix')`` for backend 'C').  ``variogram_model='custom'`` takes the host round trip of
        the moving window.  ``last_timing`` is set.  The points and results an earlier ``execute()`` left on the device stay as they
        are."""
        self._check_backend(backend, n_closest_points)
        if n_closest_points is None:
            raise ValueError("cross_validate_window needs n_closest_points (the global form is cross_validate())")
        v = None if values is None else self._field_values(values)
        n = int(np.size(self._values()))
        k = int(n_closest_points)
        if k > n - 1:
            raise ValueError("n_closest_points = %d exceeds the number of other stations (N - 1 = %d)" % (k, n - 1))
        h = self._get_handle()
        key = self._factor_key_for(h)
        if key is None or key != getattr(self, "_factor_key", None):  # (a factored problem on the handle is this object's: it stays, with its factor)
            self._set_problem(h)
        if v is not None:
            self._max_fields = max(self._max_fields, v.shape[1])
            h.set_fields(v.T)
        try:
            with _singular_as(backend):
                zhat, ss = h.cross_validate_window(k)
            self.last_timing = h.timing()
        finally:
            if v is not None:
                h.set_fields(None)
        return (zhat if v is not None and np.ndim(values) == 2 else zhat[0]), ss

    def _spec_rows(self, style, shape, npt, specified_drift_arrays):
        """uk.py:1217-1274 / uk3d.py:1030-1095: validate + flatten the per-point specified-drift arrays."""
        if specified_drift_arrays is None:
            specified_drift_arrays = []
        rows = []
        if self.specified_drift:
            if len(specified_drift_arrays) == 0:
                raise ValueError("Must provide drift values for kriging points when using 'specified' drift capability.")
            if type(specified_drift_arrays) is not list:
                raise TypeError("Arrays for specified drift terms must be encapsulated in a list.")
            for spec in specified_drift_arrays:
                spec = np.asarray(spec)
                if style in ("grid", "masked"):
                    if spec.ndim < self._ndim:
                        raise ValueError("Dimensions of drift values array do not match specified grid dimensions.")
                    if spec.shape != shape:
                        if spec.shape == tuple(reversed(shape)):
                            spec = spec.T if self._ndim == 2 else spec.swapaxes(0, 2)
                        else:
                            raise ValueError("Dimensions of drift values array do not match specified grid dimensions.")
                else:
                    if spec.ndim != 1:
                        raise ValueError("Dimensions of drift values array do not match specified grid dimensions.")
                    if spec.shape[0] != npt:
                        raise ValueError("Number of supplied drift values in array do not match specified number of kriging points.")
                rows.append(np.asarray(spec, dtype=np.float64).ravel())
            if len(rows) != len(self.specified_drift_data_arrays):
                raise ValueError("Inconsistent number of specified drift terms supplied.")
        elif len(specified_drift_arrays) != 0:
            warnings.warn("Provided specified drift values, but 'specified' drift was not initialized during "
                          "instantiation of %s class." % type(self).__name__, RuntimeWarning)
        return rows


# =====================================================================================================
class OrdinaryKriging(_KrigingBase):
    """2D ordinary kriging (ok.py:41).  ``execute`` runs on the GPU."""

    _ndim = 2
    _backends = ("vectorized", "loop", "C", "hip")
    _mw_backends = ("loop", "C", "hip")
    _label = "2D ordinary kriging"

    def __init__(self, x, y, z, variogram_model="linear", variogram_parameters=None, variogram_function=None, nlags=6,
                 weight=False, anisotropy_scaling=1.0, anisotropy_angle=0.0, verbose=False, enable_plotting=False,
                 enable_statistics=False, coordinates_type="euclidean", exact_values=True, pseudo_inv=False,
                 pseudo_inv_type="pinv"):
        variogram_parameters = self._init_common(variogram_model, variogram_parameters, variogram_function, exact_values,
                                                 pseudo_inv, pseudo_inv_type, verbose, enable_plotting)
        if self.model is not None:  # GSTools CovModel: 2-D only, its own anisotropy (ok.py:228-239)
            if self.model.field_dim == 3:
                raise ValueError("GSTools: model dim is not 1 or 2")
            if self.model.latlon and coordinates_type == "euclidean":
                raise ValueError("GSTools: latlon models require geographic coordinates")
            anisotropy_scaling, anisotropy_angle = self.model.pykrige_anis, self.model.pykrige_angle
        if coordinates_type not in ("euclidean", "geographic"):
            raise ValueError("Only 'euclidean' and 'geographic' are valid values for coordinates-keyword.")
        self.coordinates_type = coordinates_type
        self._enable_statistics = bool(enable_statistics)
        self.X_ORIG = np.atleast_1d(np.squeeze(np.array(x, copy=True, dtype=np.float64)))
        self.Y_ORIG = np.atleast_1d(np.squeeze(np.array(y, copy=True, dtype=np.float64)))
        self.Z = np.atleast_1d(np.squeeze(np.array(z, copy=True, dtype=np.float64)))
        if self.coordinates_type == "euclidean":
            self.XCENTER = (np.amax(self.X_ORIG) + np.amin(self.X_ORIG)) / 2.0
            self.YCENTER = (np.amax(self.Y_ORIG) + np.amin(self.Y_ORIG)) / 2.0
            self.anisotropy_scaling = anisotropy_scaling
            self.anisotropy_angle = anisotropy_angle
            if self.verbose:
                print("Adjusting data for anisotropy...")
            self._adjust_stations()
        else:  # ok.py:289-304: coordinates stay as they are; anisotropy is ambiguous on the sphere
            if anisotropy_scaling != 1.0:
                warnings.warn("Anisotropy is not compatible with geographic coordinates. Ignoring user set anisotropy.",
                              UserWarning)
            self.XCENTER = self.YCENTER = 0.0
            self.anisotropy_scaling, self.anisotropy_angle = 1.0, 0.0
            self.X_ADJUSTED, self.Y_ADJUSTED = self.X_ORIG, self.Y_ORIG
            self._coords_adj = np.vstack((self.X_ORIG, self.Y_ORIG)).T
        self._set_variogram_parameters(variogram_parameters, nlags, weight)
        if type(self) is OrdinaryKriging and not self._enable_statistics:  # ok.py:360-377: statistics only on request
            self.delta = self.sigma = self.epsilon = self.Q1 = self.Q2 = self.cR = None
        elif type(self) is OrdinaryKriging and self.__dict__.get("Q1") is None:  # (verbose: _set_variogram_parameters has computed and printed them)
            self._compute_statistics()

    def _center(self):
        return [self.XCENTER, self.YCENTER]

    def _scaling(self):
        return [self.anisotropy_scaling]

    def _angle(self):
        return [self.anisotropy_angle]

    def _adjust_stations(self):
        self._coords_adj = core.adjust_for_anisotropy(np.vstack((self.X_ORIG, self.Y_ORIG)).T, self._center(),
                                                      self._scaling(), self._angle())
        self.X_ADJUSTED, self.Y_ADJUSTED = self._coords_adj.T

    def execute(self, style, xpoints, ypoints, mask=None, backend="vectorized", n_closest_points=None):
        """Kriged values and variances at a grid / masked grid / list of points (ok.py:760-1020)."""
        if self.verbose:
            print("Executing Ordinary Kriging...\n")
        if style != "grid" and style != "masked" and style != "points":
            raise ValueError("style argument must be 'grid', 'points', or 'masked'")
        self._check_backend(backend, n_closest_points)
        P = self._prepare(style, (xpoints, ypoints), mask)
        if n_closest_points is not None:
            z, ss = self._solve_moving_window(P, n_closest_points, backend)
        else:
            z, ss = self._solve(P)
        return self._finish(z, ss, style, P.shape, P.mask, backend)

    def execute_fields(self, style, xpoints, ypoints, values, mask=None, backend="vectorized", n_closest_points=None, valid=None):
        return self._execute_fields(style, (xpoints, ypoints), values, mask, backend, {}, n_closest_points, valid)

    execute_fields.__doc__ = _KrigingBase._FIELDS_DOC

    def execute_cov(self, style, xpoints, ypoints, backend="vectorized", specified_drift_arrays=None):
        return self._execute_cov(style, (xpoints, ypoints), backend, specified_drift_arrays, False)

    execute_cov.__doc__ = _KrigingBase._COV_DOC

    def execute_block(self, style, xpoints, ypoints, block_size, n_disc=4, backend="vectorized"):
        return self._execute_block(style, (xpoints, ypoints), block_size, n_disc, backend)

    execute_block.__doc__ = _KrigingBase._BLOCK_DOC

    def execute_fields_window(self, style, xpoints, ypoints, values, n_closest_points, valid=None, backend="loop"):
        return self._execute_fields_window(style, [xpoints, ypoints], values, n_closest_points, valid, backend)

    execute_fields_window.__doc__ = _KrigingBase._FIELDS_WINDOW_DOC

    def execute_block_window(self, style, xpoints, ypoints, block_size, n_closest_points, n_disc=4, backend="loop"):
        return self._execute_block_window(style, (xpoints, ypoints), block_size, n_closest_points, n_disc, backend)

    execute_block_window.__doc__ = _KrigingBase._BLOCK_WINDOW_DOC


# =====================================================================================================
class UniversalKriging(OrdinaryKriging):
    """2D universal kriging (uk.py:39): regional_linear and point_log drifts are evaluated on the
    device; external_Z, specified and functional drifts are evaluated here (they are O(npt) lookups or
    user callables) and passed as extra matrix columns / RHS rows."""

    _universal = True
    _backends = ("vectorized", "loop", "hip")
    _mw_backends = ()
    _label = "2D universal kriging"

    def __init__(self, x, y, z, variogram_model="linear", variogram_parameters=None, variogram_function=None, nlags=6,
                 weight=False, anisotropy_scaling=1.0, anisotropy_angle=0.0, drift_terms=None, point_drift=None,
                 external_drift=None, external_drift_x=None, external_drift_y=None, specified_drift=None,
                 functional_drift=None, verbose=False, enable_plotting=False, exact_values=True, pseudo_inv=False,
                 pseudo_inv_type="pinv"):
        OrdinaryKriging.__init__(self, x, y, z, variogram_model=variogram_model,
                                 variogram_parameters=variogram_parameters, variogram_function=variogram_function,
                                 nlags=nlags, weight=weight, anisotropy_scaling=anisotropy_scaling,
                                 anisotropy_angle=anisotropy_angle, verbose=verbose, enable_plotting=enable_plotting,
                                 exact_values=exact_values, pseudo_inv=pseudo_inv, pseudo_inv_type=pseudo_inv_type)
        if drift_terms is None:
            drift_terms = []
        if specified_drift is None:  # uk.py:254-257, uk3d.py:249-252: an omitted list is an EMPTY list (-> ValueError, not TypeError)
            specified_drift = []
        if functional_drift is None:
            functional_drift = []
        if self.verbose:  # uk.py:396-466
            print("Initializing drift terms...")
        self.regional_linear_drift = "regional_linear" in drift_terms
        if self.regional_linear_drift and self.verbose:
            print("Implementing regional linear drift.")
        self.external_Z_drift = "external_Z" in drift_terms
        if self.external_Z_drift:
            if external_drift is None:
                raise ValueError("Must specify external Z drift terms.")
            if external_drift_x is None or external_drift_y is None:
                raise ValueError("Must specify coordinates of external Z drift terms.")
            external_drift = np.asarray(external_drift)
            ex, ey = np.asarray(external_drift_x), np.asarray(external_drift_y)
            if external_drift.shape[0] != ey.shape[0] or external_drift.shape[1] != ex.shape[0]:
                if external_drift.shape[0] == ex.shape[0] and external_drift.shape[1] == ey.shape[0]:
                    self.external_Z_array = np.array(external_drift.T)
                else:
                    raise ValueError("External drift dimensions do not match provided x- and y-coordinate dimensions.")
            else:
                self.external_Z_array = np.array(external_drift)
            self.external_Z_array_x = np.array(ex).flatten()
            self.external_Z_array_y = np.array(ey).flatten()
            self.z_scalars = self._calculate_data_point_zscalars(self.X_ORIG, self.Y_ORIG)
            if self.verbose:
                print("Implementing external Z drift.")
        self.point_log_drift = "point_log" in drift_terms
        if self.point_log_drift:
            if point_drift is None:
                raise ValueError("Must specify location(s) and strength(s) of point drift terms.")
            raw = np.asarray(point_drift)
            # (the wells go through the same in-place centring as the prediction points, uk.py:450-459: a float32 point_drift array is rounded there)
            self._point_log_dtype = raw.dtype if raw.dtype.kind == "f" and raw.dtype.itemsize < 8 else None
            point_log = np.atleast_2d(np.squeeze(np.array(point_drift, copy=True, dtype=np.float64)))
            self._point_log_user = point_log
            self._adjust_wells()
            if self.verbose:
                print("Implementing external point-logarithmic drift; number of points =", self.point_log_array.shape[0], "\n")
        self.specified_drift = "specified" in drift_terms
        if self.specified_drift:
            if type(specified_drift) is not list:
                raise TypeError("Arrays for specified drift terms must be encapsulated in a list.")
            if len(specified_drift) == 0:
                raise ValueError("Must provide at least one drift-value array when using the 'specified' drift capability.")
            self.specified_drift_data_arrays = []
            for term in specified_drift:
                specified = np.squeeze(np.array(term, copy=True))
                if specified.size != self.X_ORIG.size:
                    raise ValueError("Must specify the drift values for each data point when using the "
                                     "'specified' drift capability.")
                self.specified_drift_data_arrays.append(specified)
        self.functional_drift = "functional" in drift_terms
        if self.functional_drift:
            if type(functional_drift) is not list:
                raise TypeError("Callables for functional drift terms must be encapsulated in a list.")
            if len(functional_drift) == 0:
                raise ValueError("Must provide at least one callable object when using the 'functional' drift capability.")
            self.functional_drift_terms = functional_drift

    def _adjust_wells(self):
        pl = self._point_log_user
        self.point_log_array = np.zeros(pl.shape)
        self.point_log_array[:, 2] = pl[:, 2]
        self.point_log_array[:, :2] = core.adjust_for_anisotropy(self._as_centred(np.vstack((pl[:, 0], pl[:, 1])).T, getattr(self, "_point_log_dtype", None)),
                                                                 self._center(), self._scaling(), self._angle())

    def _calculate_data_point_zscalars(self, x, y, type_="array"):
        return core.bilinear_zscalars(self.external_Z_array, self.external_Z_array_x, self.external_Z_array_y, x, y)

    def _regional_linear(self):
        return self.regional_linear_drift

    def _wells(self):
        return self.point_log_array if self.point_log_drift else None

    def _station_extra_cols(self):
        cols = []  # reference order after regional_linear and point_log: external_Z, specified, functional
        if self.external_Z_drift:
            cols.append(self.z_scalars)
        if self.specified_drift:
            cols.extend(self.specified_drift_data_arrays)
        if self.functional_drift:
            cols.extend(f(self.X_ADJUSTED, self.Y_ADJUSTED) for f in self.functional_drift_terms)
        return np.array(cols, dtype=np.float64) if cols else None

    def execute(self, style, xpoints, ypoints, mask=None, backend="vectorized", specified_drift_arrays=None):
        """uk.py:1090-1328."""
        if self.verbose:
            print("Executing Universal Kriging...\n")
        if style != "grid" and style != "masked" and style != "points":
            raise ValueError("style argument must be 'grid', 'points', or 'masked'")
        self._check_backend(backend, None)
        P = self._prepare(style, (xpoints, ypoints), mask, specified_drift_arrays, backend)
        z, ss = self._solve(P)
        return self._finish(z, ss, style, P.shape, P.mask, backend)

    def execute_fields(self, style, xpoints, ypoints, values, mask=None, backend="vectorized", specified_drift_arrays=None, valid=None):
        return self._execute_fields(style, (xpoints, ypoints), values, mask, backend,
                                    dict(specified_drift_arrays=specified_drift_arrays, backend=backend), valid=valid)

    execute_fields.__doc__ = _KrigingBase._FIELDS_DOC

    def execute_cov(self, style, xpoints, ypoints, backend="vectorized", specified_drift_arrays=None):
        return self._execute_cov(style, (xpoints, ypoints), backend, specified_drift_arrays, True)

    execute_cov.__doc__ = _KrigingBase._COV_DOC

    def execute_block(self, style, xpoints, ypoints, block_size, n_disc=4, backend="vectorized"):
        return self._execute_block(style, (xpoints, ypoints), block_size, n_disc, backend)

    execute_block.__doc__ = _KrigingBase._BLOCK_DOC

    def _grid_rows(self, style, axes, shape, mask, specified_drift_arrays, backend):
        rows = []
        if self.external_Z_drift:  # looked up at the ORIGINAL coordinates (uk.py:967-971): the host meshgrid, for this term only
            pts = self._meshgrid(axes)
            if mask is not None and backend != "vectorized":  # see _prepare_points
                zs = np.zeros(pts.shape[0])
                keep = ~mask
                zs[keep] = self._calculate_data_point_zscalars(pts[keep, 0], pts[keep, 1])
                rows.append(zs)
            else:
                rows.append(self._calculate_data_point_zscalars(pts[:, 0], pts[:, 1]))
        rows.extend(self._spec_rows(style, shape, int(np.prod(shape)), specified_drift_arrays))
        return np.array(rows, dtype=np.float64) if rows else None

    def _prepare_points(self, style, axes, mask, specified_drift_arrays=None, backend="vectorized", adjust=True):
        pts, shape, mask = self._points_from(style, axes, mask, columns=not adjust)
        rows = []
        if self.external_Z_drift:  # on ORIGINAL coordinates (uk.py:967-971)
            if mask is not None and backend != "vectorized":
                # the reference's loop looks the drift up point by point and skips masked points (uk.py:1034, 1061-1066), so a
                # masked point outside the drift grid does not raise there; 'vectorized' looks every point up (uk.py:967-971)
                zs = np.zeros(pts.shape[0])
                keep = ~mask
                zs[keep] = self._calculate_data_point_zscalars(pts[keep, 0], pts[keep, 1])
                rows.append(zs)
            else:
                rows.append(self._calculate_data_point_zscalars(pts[:, 0], pts[:, 1]))
        rows.extend(self._spec_rows(style, shape, pts.shape[0], specified_drift_arrays))
        if not adjust:  # (never with functional drifts: _prepare) the device adjusts the coordinates
            return pts, shape, mask, (np.array(rows, dtype=np.float64) if rows else None)
        pts_adj = core.adjust_for_anisotropy(self._as_centred(pts), self._center(), self._scaling(), self._angle())
        if self.functional_drift:
            rows.extend(np.asarray(f(pts_adj[:, 0], pts_adj[:, 1]), dtype=np.float64) for f in self.functional_drift_terms)
        return pts_adj, shape, mask, (np.array(rows, dtype=np.float64) if rows else None)


# =====================================================================================================
class OrdinaryKriging3D(_KrigingBase):
    """3D ordinary kriging (ok3d.py:40)."""

    _ndim = 3
    _mw_backends = ("loop", "hip")
    _label = "3D ordinary kriging"

    def __init__(self, x, y, z, val, variogram_model="linear", variogram_parameters=None, variogram_function=None,
                 nlags=6, weight=False, anisotropy_scaling_y=1.0, anisotropy_scaling_z=1.0, anisotropy_angle_x=0.0,
                 anisotropy_angle_y=0.0, anisotropy_angle_z=0.0, verbose=False, enable_plotting=False,
                 exact_values=True, pseudo_inv=False, pseudo_inv_type="pinv"):
        variogram_parameters = self._init_common(variogram_model, variogram_parameters, variogram_function, exact_values,
                                                 pseudo_inv, pseudo_inv_type, verbose, enable_plotting)
        if self.model is not None:  # GSTools CovModel: 3-D only here, its own anisotropy (ok3d.py:232-245)
            if self.model.field_dim < 3:
                raise ValueError("GSTools: model dim is not 3")
            anisotropy_scaling_y, anisotropy_scaling_z = self.model.pykrige_anis_y, self.model.pykrige_anis_z
            anisotropy_angle_x, anisotropy_angle_y, anisotropy_angle_z = (self.model.pykrige_angle_x, self.model.pykrige_angle_y,
                                                                          self.model.pykrige_angle_z)
        self.X_ORIG = np.atleast_1d(np.squeeze(np.array(x, copy=True, dtype=np.float64)))
        self.Y_ORIG = np.atleast_1d(np.squeeze(np.array(y, copy=True, dtype=np.float64)))
        self.Z_ORIG = np.atleast_1d(np.squeeze(np.array(z, copy=True, dtype=np.float64)))
        self.VALUES = np.atleast_1d(np.squeeze(np.array(val, copy=True, dtype=np.float64)))
        self.XCENTER = (np.amax(self.X_ORIG) + np.amin(self.X_ORIG)) / 2.0
        self.YCENTER = (np.amax(self.Y_ORIG) + np.amin(self.Y_ORIG)) / 2.0
        self.ZCENTER = (np.amax(self.Z_ORIG) + np.amin(self.Z_ORIG)) / 2.0
        self.anisotropy_scaling_y = anisotropy_scaling_y
        self.anisotropy_scaling_z = anisotropy_scaling_z
        self.anisotropy_angle_x = anisotropy_angle_x
        self.anisotropy_angle_y = anisotropy_angle_y
        self.anisotropy_angle_z = anisotropy_angle_z
        if self.verbose:
            print("Adjusting data for anisotropy...")
        self._adjust_stations()
        self._set_variogram_parameters(variogram_parameters, nlags, weight)

    def _center(self):
        return [self.XCENTER, self.YCENTER, self.ZCENTER]

    def _scaling(self):
        return [self.anisotropy_scaling_y, self.anisotropy_scaling_z]

    def _angle(self):
        return [self.anisotropy_angle_x, self.anisotropy_angle_y, self.anisotropy_angle_z]

    def _adjust_stations(self):
        self._coords_adj = core.adjust_for_anisotropy(np.vstack((self.X_ORIG, self.Y_ORIG, self.Z_ORIG)).T,
                                                      self._center(), self._scaling(), self._angle())
        self.X_ADJUSTED, self.Y_ADJUSTED, self.Z_ADJUSTED = self._coords_adj.T

    def update_variogram_model(self, variogram_model, variogram_parameters=None, variogram_function=None, nlags=6,
                               weight=False, anisotropy_scaling_y=1.0, anisotropy_scaling_z=1.0, anisotropy_angle_x=0.0,
                               anisotropy_angle_y=0.0, anisotropy_angle_z=0.0):
        """ok3d.py:368-380 / uk3d.py:452-464: same signature, same (isotropic) defaults."""
        self._update_variogram_model(variogram_model, variogram_parameters, variogram_function, nlags, weight,
                                     dict(anisotropy_scaling_y=anisotropy_scaling_y, anisotropy_scaling_z=anisotropy_scaling_z,
                                          anisotropy_angle_x=anisotropy_angle_x, anisotropy_angle_y=anisotropy_angle_y,
                                          anisotropy_angle_z=anisotropy_angle_z))

    def execute(self, style, xpoints, ypoints, zpoints, mask=None, backend="vectorized", n_closest_points=None):
        """ok3d.py:735-932.  Output shape (nz, ny, nx) for grids."""
        if self.verbose:
            print("Executing Ordinary Kriging...\n")
        if style != "grid" and style != "masked" and style != "points":
            raise ValueError("style argument must be 'grid', 'points', or 'masked'")
        self._check_backend(backend, n_closest_points)
        P = self._prepare(style, (xpoints, ypoints, zpoints), mask)
        if n_closest_points is not None:
            z, ss = self._solve_moving_window(P, n_closest_points, backend)
        else:
            z, ss = self._solve(P)
        return self._finish(z, ss, style, P.shape, P.mask, backend)

    def execute_fields(self, style, xpoints, ypoints, zpoints, values, mask=None, backend="vectorized", n_closest_points=None, valid=None):
        return self._execute_fields(style, (xpoints, ypoints, zpoints), values, mask, backend, {}, n_closest_points, valid)

    execute_fields.__doc__ = _KrigingBase._FIELDS_DOC

    def execute_cov(self, style, xpoints, ypoints, zpoints, backend="vectorized", specified_drift_arrays=None):
        return self._execute_cov(style, (xpoints, ypoints, zpoints), backend, specified_drift_arrays, False)

    execute_cov.__doc__ = _KrigingBase._COV_DOC

    def execute_block(self, style, xpoints, ypoints, zpoints, block_size, n_disc=4, backend="vectorized"):
        return self._execute_block(style, (xpoints, ypoints, zpoints), block_size, n_disc, backend)

    execute_block.__doc__ = _KrigingBase._BLOCK_DOC

    def execute_fields_window(self, style, xpoints, ypoints, zpoints, values, n_closest_points, valid=None, backend="loop"):
        return self._execute_fields_window(style, [xpoints, ypoints, zpoints], values, n_closest_points, valid, backend)

    execute_fields_window.__doc__ = _KrigingBase._FIELDS_WINDOW_DOC

    def execute_block_window(self, style, xpoints, ypoints, zpoints, block_size, n_closest_points, n_disc=4, backend="loop"):
        return self._execute_block_window(style, (xpoints, ypoints, zpoints), block_size, n_closest_points, n_disc, backend)

    execute_block_window.__doc__ = _KrigingBase._BLOCK_WINDOW_DOC


# =====================================================================================================
class UniversalKriging3D(OrdinaryKriging3D):
    """3D universal kriging (uk3d.py:39): regional_linear on the device, specified / functional drifts
    evaluated on the host."""

    _universal = True
    _mw_backends = ()
    _label = "3D universal kriging"

    def __init__(self, x, y, z, val, variogram_model="linear", variogram_parameters=None, variogram_function=None,
                 nlags=6, weight=False, anisotropy_scaling_y=1.0, anisotropy_scaling_z=1.0, anisotropy_angle_x=0.0,
                 anisotropy_angle_y=0.0, anisotropy_angle_z=0.0, drift_terms=None, specified_drift=None,
                 functional_drift=None, verbose=False, enable_plotting=False, exact_values=True, pseudo_inv=False,
                 pseudo_inv_type="pinv"):
        OrdinaryKriging3D.__init__(self, x, y, z, val, variogram_model=variogram_model,
                                   variogram_parameters=variogram_parameters, variogram_function=variogram_function,
                                   nlags=nlags, weight=weight, anisotropy_scaling_y=anisotropy_scaling_y,
                                   anisotropy_scaling_z=anisotropy_scaling_z, anisotropy_angle_x=anisotropy_angle_x,
                                   anisotropy_angle_y=anisotropy_angle_y, anisotropy_angle_z=anisotropy_angle_z,
                                   verbose=verbose, enable_plotting=enable_plotting, exact_values=exact_values,
                                   pseudo_inv=pseudo_inv, pseudo_inv_type=pseudo_inv_type)
        if drift_terms is None:
            drift_terms = []
        if specified_drift is None:  # uk.py:254-257, uk3d.py:249-252: an omitted list is an EMPTY list (-> ValueError, not TypeError)
            specified_drift = []
        if functional_drift is None:
            functional_drift = []
        if self.verbose:  # uk3d.py:396-406
            print("Initializing drift terms...")
            if "regional_linear" in drift_terms:
                print("Implementing regional linear drift.")
        self.regional_linear_drift = "regional_linear" in drift_terms
        self.specified_drift = "specified" in drift_terms
        if self.specified_drift:
            if type(specified_drift) is not list:
                raise TypeError("Arrays for specified drift terms must be encapsulated in a list.")
            if len(specified_drift) == 0:
                raise ValueError("Must provide at least one drift-value array when using the 'specified' drift capability.")
            self.specified_drift_data_arrays = []
            for term in specified_drift:
                specified = np.squeeze(np.array(term, copy=True))
                if specified.size != self.X_ORIG.size:
                    raise ValueError("Must specify the drift values for each data point when using the "
                                     "'specified' drift capability.")
                self.specified_drift_data_arrays.append(specified)
        self.functional_drift = "functional" in drift_terms
        if self.functional_drift:
            if type(functional_drift) is not list:
                raise TypeError("Callables for functional drift terms must be encapsulated in a list.")
            if len(functional_drift) == 0:
                raise ValueError("Must provide at least one callable object when using the 'functional' drift capability.")
            self.functional_drift_terms = functional_drift

    def _regional_linear(self):
        return self.regional_linear_drift

    def _station_extra_cols(self):
        cols = []
        if self.specified_drift:
            cols.extend(self.specified_drift_data_arrays)
        if self.functional_drift:
            cols.extend(f(self.X_ADJUSTED, self.Y_ADJUSTED, self.Z_ADJUSTED) for f in self.functional_drift_terms)
        return np.array(cols, dtype=np.float64) if cols else None

    def execute(self, style, xpoints, ypoints, zpoints, mask=None, backend="vectorized", specified_drift_arrays=None):
        """uk3d.py:877-1146."""
        if self.verbose:
            print("Executing Universal Kriging...\n")
        if style != "grid" and style != "masked" and style != "points":
            raise ValueError("style argument must be 'grid', 'points', or 'masked'")
        self._check_backend(backend, None)
        P = self._prepare(style, (xpoints, ypoints, zpoints), mask, specified_drift_arrays)
        z, ss = self._solve(P)
        return self._finish(z, ss, style, P.shape, P.mask, backend)

    def execute_fields(self, style, xpoints, ypoints, zpoints, values, mask=None, backend="vectorized", specified_drift_arrays=None, valid=None):
        return self._execute_fields(style, (xpoints, ypoints, zpoints), values, mask, backend,
                                    dict(specified_drift_arrays=specified_drift_arrays), valid=valid)

    execute_fields.__doc__ = _KrigingBase._FIELDS_DOC

    def execute_cov(self, style, xpoints, ypoints, zpoints, backend="vectorized", specified_drift_arrays=None):
        return self._execute_cov(style, (xpoints, ypoints, zpoints), backend, specified_drift_arrays, True)

    execute_cov.__doc__ = _KrigingBase._COV_DOC

    def execute_block(self, style, xpoints, ypoints, zpoints, block_size, n_disc=4, backend="vectorized"):
        return self._execute_block(style, (xpoints, ypoints, zpoints), block_size, n_disc, backend)

    execute_block.__doc__ = _KrigingBase._BLOCK_DOC

    def _grid_rows(self, style, axes, shape, mask, specified_drift_arrays, backend):
        rows = self._spec_rows(style, shape, int(np.prod(shape)), specified_drift_arrays)
        return np.array(rows, dtype=np.float64) if rows else None

    def _prepare_points(self, style, axes, mask, specified_drift_arrays=None, backend="vectorized", adjust=True):
        pts, shape, mask = self._points_from(style, axes, mask, columns=not adjust)
        rows = self._spec_rows(style, shape, pts.shape[0], specified_drift_arrays)
        if not adjust:  # (never with functional drifts: _prepare) the device adjusts the coordinates
            return pts, shape, mask, (np.array(rows, dtype=np.float64) if rows else None)
        pts_adj = core.adjust_for_anisotropy(self._as_centred(pts), self._center(), self._scaling(), self._angle())
        if self.functional_drift:
            rows.extend(np.asarray(f(pts_adj[:, 0], pts_adj[:, 1], pts_adj[:, 2]), dtype=np.float64)
                        for f in self.functional_drift_terms)
        return pts_adj, shape, mask, (np.array(rows, dtype=np.float64) if rows else None)
