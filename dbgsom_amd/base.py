"""Host-side estimator core: the scikit-learn surface of the reference's ``BaseSom`` with the
per-epoch hot path delegated to a backend (MI355X by default, no CPU fallback).

Mirrors ``dbgsom/BaseSom.py`` of SandroMartens/DBGSOM: same constructor parameters (spelling
``convergence_treshold`` included, :42-80), same fitted attributes, same private hot-path methods
(``_get_winning_neurons``, ``_calculate_exp_similarity``, ``_update_weights``,
``_write_accumulative_error``) so call sites and tests read like the reference's.  Topology and
growth stay on the host (``lattice.GrowingLattice`` on NetworkX); only dense distance / update
arrays go to the device.

Extra, build-only parameters (defaults keep reference behaviour):
    backend         None -> ``HipBackend()``; or a ``HotPathBackend`` instance (tests inject the
                    oracle's CPU stand-in)
    centres_layout  "compact" reproduces the reference's compacted Voronoi-centre rows (quirk
                    Q1, BaseSom.py:1045,1053); "aligned" is the mathematically intended form
    device          HIP device ordinal for the default backend
    sharded_input   False: every rank of a torch.distributed group passes the SAME full X and keeps
                    its row shard resident; True: every rank passes only ITS rows (nothing of size
                    N is ever gathered; ``labels_`` then describes the local rows); dense X only
                    (``ValueError`` for sparse X)
    init            "random" (default): four random rows of X on a 2 x 2 square, as the reference starts.  "pca"
                    (alias "linear"): the linear initialisation of SOM Toolbox / MiniSom / somoclu -- prototype
                    ``(a, b)`` of an ``initial_shape = (rows, cols)`` grid starts at ``mean + (2a/(rows-1) - 1)
                    sqrt(l1) e1 + (2b/(cols-1) - 1) sqrt(l2) e2`` in float64, ``l1 >= l2`` the two largest
                    eigenvalues of the population covariance of X and ``e1``, ``e2`` their unit eigenvectors (largest
                    entry positive), found on the device by a block subspace iteration over the resident rows
                    (``dbgsom_amd.linear_init``).  ``random_state`` plays no part in that start.  Growth and everything
                    after the start are unchanged; with ``max_neurons <= rows * cols`` the map keeps its shape: a
                    fixed-grid batch SOM.  Fitted attributes under "pca" only: ``init_mean_`` (d,),
                    ``init_directions_`` (2, d), ``init_variances_`` (2,), ``init_n_passes_``.  Refused
                    (``ValueError`` in ``fit``): sparse X, NaN under ``missing_values="nan-fit"``, ``sample_weight``,
                    ``vertical_growth=True``, ``sharded_input`` or more than one rank, X with fewer than two
                    directions of variance.  Host arrays and device tensors both work.
    initial_shape   (rows, cols) of the start grid, both >= 2; anything but (2, 2) needs ``init="pca"``

Sparse input: ``fit``, ``predict``, ``transform``, ``predict_proba`` and ``calculate_quantization_error``
take a scipy sparse matrix (converted to CSR; never densified as a whole).  A fit on sparse X equals the fit
on ``X.toarray()`` up to the column moments, which are taken in float64 from the stored entries.
``topographic_function`` takes dense X only (``TypeError`` for sparse X).

Device arrays: every method that takes complete dense rows also takes a ``torch.Tensor`` that lives on the
estimator's GPU (anything ``backend.is_device_array`` accepts) and gives the result of the same call on
``X.cpu().numpy()`` bit for bit, without X crossing PCIe.  Per-row results (``predict``, ``fit_predict``,
``transform``, ``predict_proba``) come back as tensors on X's device, scalars as Python floats, fitted attributes
stay NumPy; ``SomClassifier.predict`` returns a NumPy array of class labels.  float32 / float64 rows are used as
they are (borrowed during ``fit`` when they have a multiple of 16 features, contiguous rows and a 16-byte aligned
base -- do not write to the tensor until ``fit`` returns --, copied on the device otherwise); float16 / bfloat16
rows are widened with ``.float()`` (an N x d x 4 byte device copy), integer and bool rows with ``.double()``.
Refused, with a message that says to pass a host array: a tensor on another GPU, a sparse tensor, a tensor with
NaN under ``missing_values="nan"`` / ``"nan-fit"``, more than one rank or ``sharded_input=True``, and
``predict`` / ``predict_proba`` of a classifier fitted with ``vertical_growth=True``.
"""
from __future__ import annotations

import copy
import numbers
from math import fsum, log, pi, sqrt

import networkx as nx
import numpy as np
import scipy.spatial.distance
import scipy.stats
from sklearn.base import BaseEstimator, clone
from sklearn.utils import check_array, check_random_state
from sklearn.utils.validation import check_is_fitted

from . import schedule
from ._native import MAX_MIXTURE_VALUES, MAX_NEIGHBORS, MAX_RADII, MAX_SCAN_FEATURES
from .backend import (RESIDENT, HotPathBackend, array_namespace, dist_info, dtype_name, is_device_array, is_sparse,
                      shard_bounds, squared_thresholds)
from .lattice import GrowingLattice


class DeviceSamples:
    """Samples that live in HBM only (a Voronoi subset gathered on the device, or the caller's device array
    adopted by ``load_device``): what ``fit`` and ``predict`` see in place of a NumPy array.  Carries shape and
    dtype; rows are fetched on demand.  ``source``: the caller's validated device array, kept alive (and, when
    borrowed, read in place) for as long as the fit runs; None for a subset."""

    def __init__(self, backend, source=None):
        self.backend = backend
        self.source = source
        self.shape = (backend.n_samples, backend._d)
        self.dtype = backend._x_np_dtype if not isinstance(backend._x_np_dtype, str) else np.dtype(np.float32)
        self.ndim = 2

    def __len__(self):
        return self.shape[0]


class BaseSom(BaseEstimator):
    def __init__(
        self,
        n_iter: int = 200,
        convergence_iter: int = 1,
        spreading_factor: float = 0.5,
        sigma_start=None,
        sigma_end=None,
        vertical_growth: bool = False,
        decay_function: str = "exponential",
        learning_rate: float = 0.02,
        verbose: bool = False,
        coarse_training_frac: float = 0.5,
        random_state=None,
        convergence_treshold: float = 10 ** -5,
        max_neurons: int = 100,
        metric: str = "euclidean",
        threshold_method: str = "se",
        growth_criterion: str = "quantization_error",
        min_samples_vertical_growth: int = 100,
        n_jobs: int = 1,
        backend=None,
        centres_layout: str = "compact",
        device=None,
        sharded_input: bool = False,
        init: str = "random",
        initial_shape=(2, 2),
        missing_values=None,
    ) -> None:
        self.n_iter = n_iter
        self.convergence_iter = convergence_iter
        self.spreading_factor = spreading_factor
        self.sigma_start = sigma_start
        self.sigma_end = sigma_end
        self.vertical_growth = vertical_growth
        self.decay_function = decay_function
        self.learning_rate = learning_rate
        self.verbose = verbose
        self.coarse_training_frac = coarse_training_frac
        self.random_state = random_state
        self.convergence_treshold = convergence_treshold
        self.max_neurons = max_neurons
        self.metric = metric  # read by the BMU search alone: "manhattan" / "cityblock" / "l1" is the L1 search, "cosine"
        #                       the cosine search, every other string the Euclidean one (BaseSom._search_metric); the
        #                       update is the same
        self.threshold_method = threshold_method
        self.growth_criterion = growth_criterion
        self.min_samples_vertical_growth = min_samples_vertical_growth
        self.n_jobs = n_jobs
        self.backend = backend
        self.centres_layout = centres_layout
        self.device = device
        self.sharded_input = sharded_input
        self.init = init
        self.initial_shape = initial_shape
        self.missing_values = missing_values

    # ------------------------------------------------------------------------------------------
    # backend plumbing
    # ------------------------------------------------------------------------------------------
    def _make_backend(self) -> HotPathBackend:
        if self.backend is None:
            from .backend import HipBackend

            return HipBackend(self.device)  # raises without the built extension / a GPU
        if isinstance(self.backend, HotPathBackend):
            return self.backend
        raise TypeError("backend must be None or a HotPathBackend instance")

    def _engine(self) -> HotPathBackend:
        be = getattr(self, "_backend_obj", None)
        if be is None:
            be = self._backend_obj = self._make_backend()
        return be

    def __getstate__(self):
        state = super().__getstate__() if hasattr(super(), "__getstate__") else self.__dict__.copy()
        state = dict(state)
        state.pop("_backend_obj", None)  # device handles are not picklable
        state.pop("_resident", None)
        state.pop("_index", None)        # (the index of index_rows is device state: it goes with the backend)
        for k in ("_sw", "_sw_global"):
            state.pop(k, None)
        return state

    # ------------------------------------------------------------------------------------------
    # fit
    # ------------------------------------------------------------------------------------------
    def fit(self, X, y=None, sample_weight=None):
        """Train the map on X (BaseSom.fit, BaseSom.py:88-131).

        sample_weight : array-like of shape (n_samples,), optional
            A row of weight w counts as w copies of that row: for integer weights the fit equals the
            fit on ``np.repeat(X, sample_weight, axis=0)`` for the same ``random_state`` -- start
            prototypes, growing threshold, every epoch's sums, errors, hit counts, labels and class
            frequencies -- while the BMU search and the stream of X are paid once per distinct row.
            Rows of weight 0 take no part in anything.  Non-negative, finite, not all zero, at least
            four rows of positive weight.  ``None``: every row counts once (the unweighted code path).
            ``predict`` / ``transform`` and the other queries on new data are not weighted.

        Under ``missing_values=None`` and ``"nan"`` X must be complete (``"nan"`` opens only the queries on a
        fitted map to rows with missing entries).  ``missing_values="nan-fit"``: NaN in dense X marks a missing
        entry in ``fit`` as well.  Without any NaN the fit is the ordinary one, bit for bit.  With at least one,
        every row -- complete ones included -- goes through the search over its observed entries
        (``sqrt(d / n_obs * sum over observed (x - w)^2)``, float64, direct form), the epoch sums run per
        (neuron, feature) over the rows that observe the feature, and the smoothing divides per (neuron, feature):
        ``W'_jc = sum_l h_jl A_lc C_lc / sum_l h_jl A_lc`` with A the observation counts and C = S / K the centres;
        an entry whose denominator is 0 keeps its value.  That is the aligned form of the update, always:
        ``centres_layout`` is not consulted (the compacted layout has no per-feature meaning).  The variance
        behind gamma, the "se" threshold and the start rows use ``np.nanvar`` / ``np.nanstd(ddof=1)`` /
        ``np.nanmean`` for the start rows' holes.  Refused (``ValueError``): an infinity, a row without any
        observed entry, a column with fewer than two observed values, ``sample_weight``,
        ``vertical_growth=True``, ``sharded_input`` or more than one rank, sparse X with a stored NaN.

        X may be a device array (a ``torch.Tensor`` on the estimator's GPU, complete rows): the fit is the fit on
        ``X.cpu().numpy()`` bit for bit and X never crosses PCIe.  A float32 / float64 tensor of a multiple of 16
        features with contiguous rows and a 16-byte aligned base is read in place for the whole fit: do not write
        to it until ``fit`` returns.  ``y`` and ``sample_weight`` may be host arrays or tensors (they go to the
        host)."""
        self._accepts_nan()   # (validates the parameter)
        self._incomplete_fit = False
        self._metric_fit = None
        self._index = None        # (the rows index_rows made resident are replaced)
        if isinstance(X, DeviceSamples):   # a Voronoi subset that already lives in HBM (f-4)
            if y is not None:
                y = np.asarray(y)
            if sample_weight is not None:
                sample_weight = np.ascontiguousarray(sample_weight, dtype=np.float64)
        else:
            X, y = self._check_input_data(X, y)
            self._check_init_fit(X, sample_weight)
            self._metric_fit = self._check_metric_fit(X, sample_weight)
            self._incomplete_fit = self._check_incomplete_fit(X, sample_weight)
            sample_weight = self._check_sample_weight(sample_weight, X)
        if self.growth_criterion == "target_error" and not self._GROWS_ON_TARGETS:
            raise ValueError(f"growth_criterion='target_error' needs a continuous target: it is SomRegressor's; "
                             f"{type(self).__name__} takes 'quantization_error' or 'entropy'")
        if y is not None:
            y = self._encode_targets(y)
        self.random_state_ = check_random_state(self.random_state)
        engine = self._engine()
        if is_device_array(X):
            # rows that are in HBM already: adopted where they are (or pad-copied on the device), and from here on
            # the fit is the one vertical-growth children run on their device subsets
            if not hasattr(engine, "load_device"):
                raise TypeError(f"the {engine.name} backend takes host arrays only: pass X.cpu().numpy()")
            engine.load_device(X)
            X = DeviceSamples(engine, source=X)
        self._load_resident(X)  # samples go to HBM once and stay there for the whole fit
        try:
            if self._metric_fit:
                engine.set_metric(self._metric_fit)   # (the search of the resident rows, until the release below)
            self._attach_sample_weight(X, sample_weight)
            self._initialize_som(X)
            self._grow_som(X, y)
            self.topographic_error_ = self._calculate_topographic_error(X)
            self.quantization_error_ = self.calculate_quantization_error(X)
            self.n_features_in_ = X.shape[1]
            self._write_node_statistics(X)
            self._delete_dead_neurons_from_graph(X)
            self._label_prototypes(X, y)
            if self.vertical_growth:
                self._grow_vertical(X, y)
            self._fit(X)
            self.n_iter_ = self._current_epoch
        finally:
            self._resident = None
            self._incomplete_fit = False
            if self._metric_fit:
                self._metric_fit = None
                engine.set_metric("euclidean")   # (the backend object may serve another fit)
            self._sw = self._sw_global = None
            if hasattr(engine, "set_sample_weight") and getattr(engine, "_sw", None) is not None:
                engine.set_sample_weight(None)   # (the backend object may serve another fit)
            if getattr(engine, "_targets", None) is not None:
                engine.set_targets(None)
            engine.release()
        return self

    _GROWS_ON_TARGETS = False   # growth_criterion="target_error" (SomRegressor)

    def _encode_targets(self, y):
        """What ``fit`` makes of y before the map is trained -> the y handed on to ``_grow_som``, ``_label_prototypes``
        and ``_grow_vertical``.  Default: class codes, the classes in ``classes_``."""
        classes, y = np.unique(y, return_inverse=True)
        self.classes_ = np.array(classes)
        return y

    # -- metric="manhattan", metric="cosine" -------------------------------------------------------------
    _MANHATTAN = ("manhattan", "cityblock", "l1")
    _COSINE = ("cosine",)
    _METRIC_LABEL = {"manhattan": "Manhattan", "cosine": "cosine"}
    _metric_fit = None    # the metric this fit runs under when it is not the Euclidean one: "manhattan" or "cosine"

    def _search_metric(self):
        """The metric of the best-matching-unit search when it is not the Euclidean one, else None.  "manhattan",
        "cityblock" and "l1" name the L1 search, ``dist(x, w) = sum_k |x_k - w_k|`` in float64; "cosine" the cosine
        search, ``1 - <x, w> / (|x| |w|)`` in float64 (a zero row is at distance 1 from everything).  ``metric`` must
        be a string; every other string is the Euclidean search as ever."""
        if not isinstance(self.metric, str):
            raise ValueError(f"metric must be a string, got {self.metric!r}")
        if self.metric in self._MANHATTAN:
            return "manhattan"
        if self.metric in self._COSINE:
            return "cosine"
        return None

    def _refuse_metric(self, kind: str, what: str, way_out: str = "") -> None:
        raise ValueError(f"metric={self.metric!r} ({self._METRIC_LABEL[kind]}) does not support {what}"
                         + (f": {way_out}" if way_out else ""))

    def _check_metric_query(self, kind: str, X) -> None:
        """The refusals of a query under the Manhattan or the cosine metric, on the host before anything is uploaded.
        (A device array never holds NaN here: ``_check_device_array`` has refused it, under ``missing_values`` by
        name.)"""
        if is_sparse(X):
            self._refuse_metric(kind, "scipy sparse X", "pass X.toarray()")
        if self._accepts_nan() and isinstance(X, np.ndarray) and np.isnan(X).any():
            self._refuse_metric(kind, f"rows with missing entries (missing_values={self.missing_values!r} and NaN in X)",
                                "impute them first, or use metric='euclidean'")

    def _check_metric_fit(self, X, sample_weight):
        """The metric this fit runs under when it is not the Euclidean one, else None; its refusals, on the host
        before anything is uploaded."""
        kind = self._search_metric()
        if kind is None:
            return None
        self._check_metric_query(kind, X)
        if sample_weight is not None:
            self._refuse_metric(kind, "sample_weight", "repeat the rows instead (np.repeat(X, w, axis=0))")
        if self.vertical_growth:
            self._refuse_metric(kind, "vertical_growth=True")
        if self.sharded_input or dist_info()[1] > 1:
            self._refuse_metric(kind, "sharded_input or a process group of more than one rank", "it takes one process")
        return kind

    # -- init="pca", initial_shape ----------------------------------------------------------------------
    _PCA_INIT = ("pca", "linear")

    def _init_kind(self) -> str:
        """"random" or "pca" (its alias "linear" included); validates ``init`` and ``initial_shape``."""
        if self.init == "random":
            kind = "random"
        elif isinstance(self.init, str) and self.init in self._PCA_INIT:
            kind = "pca"
        else:
            raise ValueError(f"init must be 'random' or 'pca' (alias 'linear'), got {self.init!r}")
        shape = self.initial_shape
        try:
            ok = len(shape) == 2 and all(isinstance(v, numbers.Integral) and not isinstance(v, bool) and v >= 2
                                         for v in shape)
        except TypeError:
            ok = False
        if not ok:
            raise ValueError(f"initial_shape must be (rows, cols), both integers >= 2, got {shape!r}")
        if kind == "random" and tuple(int(v) for v in shape) != (2, 2):
            raise ValueError(f"initial_shape={shape!r} needs init=\"pca\": init={self.init!r} starts from a 2 x 2 square "
                             "of four random rows")
        return kind

    def _refuse_pca(self, what: str, way_out: str = "") -> None:
        raise ValueError(f'init="pca" does not support {what}' + (f": {way_out}" if way_out else ""))

    def _check_init_fit(self, X, sample_weight) -> None:
        """The refusals of the linear initialisation, on the host before anything is uploaded."""
        if self._init_kind() != "pca":
            return
        if is_sparse(X):
            self._refuse_pca("scipy sparse X", "pass X.toarray(), or use init='random'")
        if self._fits_nan() and isinstance(X, np.ndarray) and np.isnan(X).any():
            self._refuse_pca(f"rows with missing entries (missing_values={self.missing_values!r} and NaN in X)",
                             "impute them first, or use init='random'")
        if sample_weight is not None:
            self._refuse_pca("sample_weight", "repeat the rows instead (np.repeat(X, w, axis=0))")
        if self.vertical_growth:
            self._refuse_pca("vertical_growth=True")
        if self.sharded_input or dist_info()[1] > 1:
            self._refuse_pca("sharded_input or a process group of more than one rank", "it takes one process")

    # -- rows with missing entries in fit (missing_values="nan-fit") ---------------------------------
    _incomplete_fit = False   # this fit runs in incomplete mode: X is dense and holds at least one NaN

    def _fits_nan(self) -> bool:
        return self._accepts_nan() and self.missing_values == "nan-fit"

    def _check_incomplete_fit(self, X, sample_weight) -> bool:
        """Whether this fit runs in incomplete mode; its refusals, on the host before anything is uploaded."""
        if not self._fits_nan() or is_sparse(X) or is_device_array(X):   # (a device array is complete: validated)
            return False
        holes = np.isnan(X)
        if not holes.any():
            return False
        self._incomplete_rows(X)   # (a row without any observed entry: the queries' message, which names the row)
        short = np.flatnonzero((~holes).sum(axis=0) < 2)
        if short.size:
            raise ValueError(f"column {int(short[0])} of X has fewer than two observed values: its variance is undefined")
        if sample_weight is not None:
            raise ValueError("sample_weight is not supported on rows with missing entries (missing_values='nan-fit')")
        if self.vertical_growth:
            raise ValueError("vertical_growth=True is not supported on rows with missing entries "
                             "(missing_values='nan-fit')")
        if self.sharded_input or dist_info()[1] > 1:
            raise ValueError("rows with missing entries (missing_values='nan-fit') take one process: no sharded_input, "
                             "no process group of more than one rank")
        return True

    def _check_fit_array(self, X, y=None, supervised=False):
        """check_array / check_X_y of fit's X.  ``missing_values="nan-fit"``: NaN passes in dense X, an infinity
        never does, and the finite check is not deferred to the device."""
        if is_device_array(X):
            X = self._check_device_array(X, fit=True)
            return X, (self._check_device_y(X, y) if supervised else None)
        kw = dict(ensure_min_samples=4, dtype=[np.float64, np.float32], accept_sparse="csr")
        if self._fits_nan():
            self._finite_deferred = False
            kw.update(self._finite_kw("allow-nan"))
        else:
            self._finite_deferred = self._finite_check_on_device()
            kw.update(self._finite_kw(not self._finite_deferred))
        if not supervised:
            return check_array(array=X, **kw), None
        from sklearn.utils import check_X_y

        return check_X_y(X=X, y=y, **kw)

    # -- device arrays: the counterpart of check_array, with the array's own operations on its device ----------
    def _host(self, a) -> np.ndarray:
        """A small per-row array (y, sample_weight, winners ...) on the host, whatever it was handed over as."""
        if is_device_array(a):
            engine = self._engine()
            return engine.fetch(a) if hasattr(engine, "fetch") else np.asarray(a.cpu())
        if hasattr(a, "detach") and hasattr(a, "numpy"):   # a CPU tensor
            return a.detach().numpy()
        return a

    def _like(self, a, like):
        """The host array `a` as an array next to the device array `like`."""
        engine = self._engine()
        if hasattr(engine, "put"):
            return engine.put(a, like)
        return array_namespace(like).asarray(np.ascontiguousarray(a), device=like.device)

    _HOST_ARRAY = "pass a host array instead (X.cpu().numpy())"

    def _check_device_array(self, X, fit: bool):
        """Validate rows that live in GPU memory (``backend.is_device_array``) -> the array the backend is handed:
        2-D, at least 4 rows for ``fit`` and 1 for a query, the fitted feature count for a query; float32 / float64
        kept, float16 / bfloat16 widened with ``.float()``, integers and bool with ``.double()``; unit column
        stride (``.contiguous()`` otherwise); finite.  Refusals come first, before anything is launched."""
        name = type(self).__name__
        layout = str(getattr(X, "layout", "strided"))
        if getattr(X, "is_sparse", False) or not layout.endswith("strided"):
            raise TypeError(f"{name} takes dense device arrays only; for sparse rows pass a host array instead "
                            "(a scipy CSR matrix)")
        if self.sharded_input or dist_info()[1] > 1:
            raise ValueError(f"device arrays take one process: no sharded_input, no process group of more than one "
                             f"rank; {self._HOST_ARRAY}")
        engine = self._engine()
        index, mine = getattr(X.device, "index", None), getattr(engine, "device_index", None)
        if index is not None and mine is not None and index != mine:
            raise ValueError(f"X lives on GPU {index}, this estimator runs on GPU {mine}: move it there, or "
                             f"{self._HOST_ARRAY}")
        if len(X.shape) != 2:
            raise ValueError(f"Expected 2D array, got {len(X.shape)}D array instead (shape={tuple(X.shape)})")
        n, d = int(X.shape[0]), int(X.shape[1])
        need = 4 if fit else 1
        if n < need:
            raise ValueError(f"Found array with {n} sample(s) (shape={(n, d)}) while a minimum of {need} is required.")
        if d < 1:
            raise ValueError(f"Found array with {d} feature(s) (shape={(n, d)}) while a minimum of 1 is required.")
        if not fit and d != self.n_features_in_:
            raise ValueError(f"X has {d} features, but {name} is expecting {self.n_features_in_} features as input")
        dt = dtype_name(X)
        if dt in ("float16", "bfloat16"):
            X = X.float()          # exact; an N x d x 4 byte copy on the device
        elif dt.startswith(("int", "uint", "bool")):
            X = X.double()         # as check_array converts integer input
        elif dt not in ("float32", "float64"):
            raise TypeError(f"device arrays of dtype {dt} are not supported; {self._HOST_ARRAY}")
        if X.stride(1) != 1 or (n > 1 and X.stride(0) < d):
            X = X.contiguous()
        if fit and not self._fits_nan() and self._finite_check_on_device():
            self._finite_deferred = True   # rides on the device's column sums (_assert_finite_from_moments)
        else:
            self._finite_deferred = False
            self._device_assert_finite(X)
        return X

    def _device_assert_finite(self, X) -> None:
        """sklearn's "no NaN, no infinity" on a device array: one reduction on the device, its ValueError."""
        ns = array_namespace(X)
        if bool(ns.isfinite(X).all()):
            return
        has_nan = bool(ns.isnan(X).any())
        if has_nan and self._accepts_nan():
            raise ValueError(f"X holds NaN: rows with missing entries (missing_values={self.missing_values!r}) are "
                             f"taken from host arrays only; {self._HOST_ARRAY}")
        from sklearn.utils import assert_all_finite

        np_dtype = np.float32 if dtype_name(X) == "float32" else np.float64
        assert_all_finite(np.array([np.nan if has_nan else np.inf], dtype=np_dtype))   # (raises, in sklearn's words)

    def _check_device_y(self, X, y) -> np.ndarray:
        """What check_X_y does for y next to a device array X: y on the host, 1-D, finite, one per row."""
        from sklearn.utils import assert_all_finite, column_or_1d

        if y is None:
            raise ValueError(f"{type(self).__name__} requires y to be passed, but the target y is None")
        y = column_or_1d(np.asarray(self._host(y)), warn=True)
        if y.dtype.kind in "fc":
            assert_all_finite(y, input_name="y")
        if y.shape[0] != X.shape[0]:
            raise ValueError(f"Found input variables with inconsistent numbers of samples: "
                             f"{[int(X.shape[0]), int(y.shape[0])]}")
        return y

    # -- sample weights -------------------------------------------------------------------------
    _sw = None          # the weights of the rows handed to fit (None: unweighted), aligned with X as passed
    _sw_global = None   # the weights of all rows of all ranks (differs from _sw with sharded_input only)
    _w_total = None     # their sum
    _w_integer = None   # every weight is an integer (the start rows are then those of the fit on repeated rows)
    _w_offset = None    # sharded_input, integer weights: the summed weight of the ranks before this one

    def _check_sample_weight(self, sample_weight, X):
        if sample_weight is None:
            return None
        from sklearn.utils.validation import _check_sample_weight

        w = _check_sample_weight(self._host(sample_weight), X, dtype=np.float64, ensure_non_negative=True)
        if getattr(self, "_finite_deferred", False):
            # (the finite check that rides on the device's column sums does not see rows of weight 0)
            from sklearn.utils import assert_all_finite

            self._finite_deferred = False
            if is_device_array(X):
                self._device_assert_finite(X)
            else:
                assert_all_finite(X)
        return np.ascontiguousarray(w, dtype=np.float64)

    def _attach_sample_weight(self, X, w) -> None:
        """Hand this rank's rows' weights to the backend (resident next to the samples) and keep what the
        host side needs: the weights of all rows and their sum."""
        self._sw = w
        self._sw_global = w
        self._w_total = None
        self._w_integer = self._w_offset = None
        engine = self._engine()
        if w is None:
            if hasattr(engine, "set_sample_weight") and getattr(engine, "_sw", None) is not None:
                engine.set_sample_weight(None)   # (a backend that an earlier, weighted fit used)
            return
        if isinstance(X, DeviceSamples):
            if not getattr(engine, "_weighted", False):   # (a device subset brings its rows' weights along)
                engine.set_sample_weight(w)
        elif self._local_input():
            engine.set_sample_weight(w)
        else:
            lo, hi = self._shard
            engine.set_sample_weight(w[lo:hi])
        # sum w, rows of positive weight, rows whose weight is no integer: all-reduced once per fit when every rank
        # holds its own rows only
        tot = np.array([w.sum(), np.count_nonzero(w > 0), np.count_nonzero(w != np.floor(w))], dtype=np.float64)
        if self._local_input():
            local_total = tot[0]
            tot = self._all_reduce_f64(tot)
        self._w_total, positive, self._w_integer = float(tot[0]), int(tot[1]), tot[2] == 0
        if not self._w_total > 0:
            raise ValueError("sample_weight is all zero")
        if positive < 4:
            raise ValueError(f"Found array with {positive} sample(s) of positive weight "
                             "while a minimum of 4 is required.")
        if self._local_input():
            if self._w_integer:
                # where this rank's copies begin among the sum w copies of all ranks: an exclusive scan of the totals
                rank = dist_info()[0]
                self._w_offset = int(sum(self._all_gather_ints(int(round(local_total)))[:rank]))
            else:
                # (a draw with probabilities w / sum w needs every weight: 8 bytes per row of the whole data set, gathered
                #  for fractional weights only)
                import torch.distributed as td

                parts = [None] * td.get_world_size()
                td.all_gather_object(parts, w)
                self._sw_global = np.concatenate(parts)

    def _n_effective(self):
        """What "how many rows" means for this fit: their number, or the summed weight."""
        return self._n_total if self._sw is None else self._w_total

    def _load_resident(self, X) -> None:
        """Make this rank's rows resident in HBM.  Default: every rank holds the same X and
        uploads its contiguous row shard (one process per GPU); ``sharded_input``: X already is
        this rank's shard; a ``DeviceSamples`` is resident as it is."""
        rank, world = dist_info()
        self._n_total = int(X.shape[0])
        if isinstance(X, DeviceSamples):
            self._shard = (0, X.shape[0])
        elif self.sharded_input and world > 1:
            sizes = self._all_gather_ints(X.shape[0])
            lo = int(sum(sizes[:rank]))
            self._shard = (lo, lo + X.shape[0])     # position of the local rows in the global order
            self._n_total = int(sum(sizes))
            self._engine().load(X)
        else:
            self._shard = shard_bounds(X.shape[0], rank, world)
            if self._incomplete_fit:
                self._engine().load(X, incomplete=True)
            else:
                self._engine().load(X[self._shard[0]:self._shard[1]])
        self._resident = X

    def _local_input(self) -> bool:
        """True when the X handed to fit holds only this rank's rows."""
        return bool(self.sharded_input) and dist_info()[1] > 1

    @staticmethod
    def _all_gather_ints(value):
        import torch
        import torch.distributed as td

        world = td.get_world_size()
        dev = "cuda" if td.get_backend() == "nccl" else "cpu"
        mine = torch.tensor([int(value)], dtype=torch.int64, device=dev)
        parts = [torch.zeros_like(mine) for _ in range(world)]
        td.all_gather(parts, mine)
        return [int(p.item()) for p in parts]

    @staticmethod
    def _all_reduce_f64(arr):
        """Element-wise sum of a small host array over the ranks."""
        import torch
        import torch.distributed as td

        t = torch.from_numpy(np.ascontiguousarray(arr, dtype=np.float64).copy())
        if td.get_backend() == "nccl":
            t = t.cuda()
        td.all_reduce(t, op=td.ReduceOp.SUM)
        return t.cpu().numpy()

    def _check_input_data(self, X, y):
        raise NotImplementedError

    def _check_sparse_input(self, X):
        """What sklearn's validation leaves to do for sparse X: the finite check on the host (a pass over the
        stored entries; nothing is deferred to the device), the modes that take dense X only, and canonical form
        (sorted column indices, duplicates summed) on a copy when X is not in it.  -> X"""
        if not is_sparse(X):
            return X
        if self.sharded_input:
            raise ValueError("sharded_input=True takes dense X only; with sparse X every rank passes the whole "
                             "matrix and keeps its row slice resident")
        self._finite_deferred = False
        from sklearn.utils import assert_all_finite

        assert_all_finite(X.data)
        if not X.has_canonical_format:   # (the column moments and the device want one stored entry per position)
            X = X.copy()
            X.sum_duplicates()
        return X

    @staticmethod
    def _sparse_column_s2(X, w=None, total=None):
        """sum_i w_i (x_ij - mean_j)^2 per column of a CSR / CSC matrix in float64 from the stored entries:
        mean_j = sum / n,  s2_j = sum over stored (x - mean_j)^2 + (n - nnz_j) mean_j^2; with weights the same
        with w_i in every sum, n = `total` = sum w and nnz_j the summed weight of the column's stored entries."""
        csr = X.tocsr()
        d = csr.shape[1]
        val = csr.data.astype(np.float64, copy=False)
        col = csr.indices
        if w is None:
            n = float(csr.shape[0])
            wv = None
            stored = np.bincount(col, minlength=d).astype(np.float64)
        else:
            n = float(total)
            wv = np.repeat(np.asarray(w, dtype=np.float64), np.diff(csr.indptr))
            stored = np.bincount(col, weights=wv, minlength=d)
        mean = np.bincount(col, weights=val if wv is None else wv * val, minlength=d) / n
        dev2 = (val - mean[col]) ** 2
        return np.bincount(col, weights=dev2 if wv is None else wv * dev2, minlength=d) + (n - stored) * mean ** 2

    # -- input validation (SomVQ.py:122 / SomClassifier.py: check_array / check_X_y) -------------
    def _finite_check_on_device(self) -> bool:
        """Whether the "no NaN, no infinity" part of sklearn's input validation can ride on the column sums
        the initialisation takes from the resident samples anyway (one host pass over X saved: 0.15 s of a
        1.3 s fit at 1e6 x 784): the default backend, one process, the whole X resident."""
        from .backend import HipBackend

        return (self.backend is None or isinstance(self.backend, HipBackend)) and dist_info()[1] == 1 \
            and not self.sharded_input

    @staticmethod
    def _finite_kw(check: bool) -> dict:
        """`ensure_all_finite` (scikit-learn >= 1.6) / `force_all_finite` (before) of check_array."""
        import inspect

        from sklearn.utils import check_array

        name = "ensure_all_finite" if "ensure_all_finite" in inspect.signature(check_array).parameters \
            else "force_all_finite"
        return {name: check}

    def _assert_finite_from_moments(self, X, mom) -> None:
        """The deferred half of the validation: a NaN or an infinity anywhere in a column shows in the column's
        sum (NaN / +-inf / NaN for +inf and -inf together).  Only when a sum is not finite is sklearn's own
        check run -- it raises its usual ValueError, or passes (finite values whose sum overflowed)."""
        if not getattr(self, "_finite_deferred", False):
            return
        self._finite_deferred = False
        if mom is None or not (np.isfinite(mom[0]).all() and np.isfinite(mom[1]).all()):
            if isinstance(X, DeviceSamples):   # the caller's device array: the same check, on the device
                self._device_assert_finite(X.source)
                return
            from sklearn.utils import assert_all_finite

            assert_all_finite(X)

    def _label_prototypes(self, X, y) -> None:
        raise NotImplementedError

    def _fit(self, X):
        pass

    def predict(self, X):
        raise NotImplementedError

    # -- initialisation (BaseSom.py:352-385, 419-444) -------------------------------------------
    def _initialize_som(self, data) -> None:
        self._current_epoch = 0
        self.converged_ = False
        self._training_phase = "coarse"
        engine = self._engine()
        rank, world = dist_info()
        n_total = self._n_total
        if self._incomplete_fit:
            # moments and start on the host, one pass each, NumPy's own dtype rules
            self._col_s2 = None
            self.growing_threshold_ = self._calculate_growing_threshold(data)
            self._total_variance = np.nanvar(data, axis=0).sum()
            self._build_lattice(*self._start_prototypes(data))
            return
        # np.var / np.std over the samples (two host passes over X, 1.4 s at 1e6 x 784) from the
        # resident copy when it is the whole data set: same values bit for bit (f-1)
        self._col_s2 = None
        on_device = isinstance(data, DeviceSamples)
        sparse = is_sparse(data)
        if sparse:
            # every rank holds the whole matrix: the moments on the host, in float64, from the stored entries
            self._col_s2 = self._sparse_column_s2(data, self._sw, self._w_total if self._sw is not None else None)
        elif self._sw is not None:
            # weighted population moments, divisor sum w: accumulated in float64 whatever the dtype of X
            wt = self._w_total
            if self._local_input():
                loc, wc = np.asarray(data, dtype=np.float64), self._sw[:, None]
                mean = self._all_reduce_f64((wc * loc).sum(axis=0)) / wt
                self._col_s2 = self._all_reduce_f64((wc * (loc - mean) ** 2).sum(axis=0))
            elif (on_device or self._shard == (0, data.shape[0])) and hasattr(engine, "weighted_column_moments"):
                self._col_s2 = engine.weighted_column_moments(wt)[1]
            else:
                # (NumPy's own axis-0 sums: with all-ones weights on float64 data, np.var's arithmetic)
                full, wc = np.asarray(data, dtype=np.float64), self._sw[:, None]
                mean = (wc * full).sum(axis=0) / wt
                self._col_s2 = (wc * (full - mean) ** 2).sum(axis=0)
        elif self._local_input():
            # every rank holds its own rows: moments from two all-reduced passes in float64 (the
            # single-process values up to float64 reassociation -- not NumPy's sequential order)
            loc = np.asarray(data, dtype=np.float64)
            mean = self._all_reduce_f64(loc.sum(axis=0)) / n_total
            self._col_s2 = self._all_reduce_f64(((loc - mean) ** 2).sum(axis=0)).astype(data.dtype)
        elif self._shard == (0, data.shape[0]) and hasattr(engine, "column_moments"):
            mom = engine.column_moments()
            if not on_device or data.source is not None:
                self._assert_finite_from_moments(data, mom)
            if mom is not None:
                self._col_s2 = mom[1]
        if getattr(self, "_finite_deferred", False):   # (no moments from the device after all: the host check now)
            self._assert_finite_from_moments(data, None)
        if self._col_s2 is None and on_device:
            raise ValueError("a DeviceSamples fit needs float32 / float64 resident samples")
        self.growing_threshold_ = self._calculate_growing_threshold(data)
        # keeps the dtype NumPy gives it: float32 data -> float32 variance -> float32 reciprocal
        if self._col_s2 is not None:
            self._total_variance = np.true_divide(self._col_s2, self._n_effective()).sum()
        else:
            self._total_variance = np.var(data, axis=0).sum()
        self._col_s2 = None
        self._build_lattice(*self._start_prototypes(data))

    _CORNERS = [(0, 0), (0, 1), (1, 0), (1, 1)]

    def _build_lattice(self, nodes, W) -> None:
        """The start lattice from ``_start_prototypes``' (nodes, W): the nodes are a full rows x cols rectangle in
        row-major order, W their prototypes in that order."""
        nodes = [tuple(int(v) for v in n) for n in nodes]
        rows, cols = max(a for a, _ in nodes) + 1, max(b for _, b in nodes) + 1
        if nodes != [(a, b) for a in range(rows) for b in range(cols)] or len(W) != len(nodes):
            raise ValueError("a start is a full rows x cols rectangle of nodes in row-major order, one prototype each")
        self._lattice = GrowingLattice(W) if (rows, cols) == (2, 2) else GrowingLattice.grid(rows, cols, W)
        self._sync_views(refresh_weights=True)

    def _start_prototypes(self, data):
        """The start of a fit -> (nodes, W): lattice nodes ``(a, b)`` of a rows x cols rectangle in row-major order
        and their prototypes.  ``init="random"``: four random rows of X on the 2 x 2 square, in X's dtype.
        ``init="pca"``: the ``initial_shape`` grid on the plane of the two leading principal directions of the resident
        rows, float64 (``linear_init``); sets ``init_mean_``, ``init_directions_``, ``init_variances_`` and
        ``init_n_passes_``.  ``_initialize_som`` builds the lattice from what this returns, whatever it is."""
        for name in ("init_mean_", "init_directions_", "init_variances_", "init_n_passes_"):
            if hasattr(self, name):
                delattr(self, name)
        if self._init_kind() == "pca":
            from . import linear_init

            rows, cols = (int(v) for v in self.initial_shape)
            plane = linear_init.principal_plane(self._engine(), self._n_total, int(data.shape[1]))
            self.init_mean_, self.init_directions_ = plane.mean, plane.directions
            self.init_variances_, self.init_n_passes_ = plane.variances, plane.n_passes
            nodes = [(a, b) for a in range(rows) for b in range(cols)]
            return nodes, linear_init.grid_prototypes(plane, rows, cols)
        engine = self._engine()
        rank, world = dist_info()
        n_total = self._n_total
        if self._incomplete_fit:
            rng = np.random.default_rng(seed=self.random_state)
            start = data[rng.choice(n_total, size=4, replace=False)]
            fill = np.nanmean(data, axis=0, dtype=np.float64).astype(data.dtype)
            return list(self._CORNERS), np.where(np.isnan(start), fill[None, :], start)
        on_device = isinstance(data, DeviceSamples)
        sparse = is_sparse(data)
        seed = self.random_state
        if world > 1 and seed is None:
            # every rank must start from the same four prototypes: rank 0 draws the seed
            drawn = np.random.SeedSequence().entropy % (2 ** 62) if rank == 0 else 0
            seed = int(self._all_reduce_f64(np.array([float(drawn >> 31), float(drawn & (2 ** 31 - 1))]))
                       @ np.array([2.0 ** 31, 1.0]))
        rng = np.random.default_rng(seed=seed)
        if on_device or self._local_input() or self._sw is not None or sparse:
            if self._sw is None:
                # rng.choice(a=data, size=4, replace=False) picks rows rng.choice(n, 4, replace=False)
                rows = rng.choice(n_total, size=4, replace=False)
            else:
                rows = self._draw_weighted_rows(rng)
            if sparse:
                start = data[rows].toarray()
            elif not (on_device or self._local_input()):
                start = data[rows]
            elif on_device:
                start = engine.read_samples(rows).astype(data.dtype)
            else:
                lo, hi = self._shard
                start = np.zeros((4, data.shape[1]))
                for k, r in enumerate(rows):
                    if lo <= r < hi:
                        start[k] = data[r - lo]
                start = self._all_reduce_f64(start).astype(data.dtype)   # one owner per row: exact
        else:
            start = rng.choice(a=data, size=4, replace=False)
        return list(self._CORNERS), start

    def _draw_weighted_rows(self, rng) -> np.ndarray:
        """The four start rows under weights.  All weights integers: the rows that
        rng.choice(a=np.repeat(X, w, 0), size=4, replace=False) returns -- draw from the sum w copies and
        map each draw to its owner through cumsum(w) (all ones: the unweighted start).  Otherwise four
        distinct rows with probabilities w / sum w."""
        w = self._sw_global
        if self._w_integer:
            draws = rng.choice(int(round(self._w_total)), size=4, replace=False)
            if self._w_offset is None:
                return np.searchsorted(np.cumsum(w), draws, side="right")
            # every rank holds its own rows: the owner of a draw is on the rank whose copies it falls among
            mine = draws - self._w_offset
            own = (mine >= 0) & (mine < int(round(w.sum())))
            rows = np.where(own, self._shard[0] + np.searchsorted(np.cumsum(w), np.where(own, mine, 0), side="right"), 0)
            return np.rint(self._all_reduce_f64(rows.astype(np.float64))).astype(np.int64)   # one owner per draw
        return rng.choice(w.shape[0], size=4, replace=False, p=w / self._w_total)

    def _calculate_growing_threshold(self, data: np.ndarray) -> float:
        if self.growth_criterion == "entropy":
            return self.spreading_factor
        if self.growth_criterion == "target_error":
            return self._target_growing_threshold()
        if self.threshold_method == "classical":
            return -data.shape[1] * log(self.spreading_factor)
        if self.threshold_method == "se":
            if self._incomplete_fit:
                spread = np.nanstd(data, axis=0, ddof=1)
            elif getattr(self, "_col_s2", None) is not None:
                if self._sw is not None and not self._w_total > 1:
                    raise ValueError("threshold_method='se' needs a summed sample_weight above 1 "
                                     "(frequency weights: the divisor is sum w - 1)")
                spread = np.sqrt(np.true_divide(self._col_s2, max(self._n_effective() - 1, 0)))
            else:
                spread = np.std(data, axis=0, ddof=1)
            return float(150 * -log(self.spreading_factor) * np.linalg.norm(spread))
        raise ValueError("threshold_method not supported. Must be 'se' or 'classical'.")

    def _target_growing_threshold(self) -> float:
        """``growing_threshold_`` under ``growth_criterion="target_error"``: the formula of the quantization-error
        criterion with the targets in the place of X -- "se": ``150 * -log(spreading_factor) * ||std(y, ddof=1)||_2``
        (weighted: divisor ``sum w - 1``, in float64), "classical": ``-T * log(spreading_factor)``."""
        Y = self._fit_targets
        if self.threshold_method == "classical":
            return -Y.shape[1] * log(self.spreading_factor)
        if self.threshold_method == "se":
            if self._sw is None:
                spread = np.std(Y, axis=0, ddof=1)
            else:
                if not self._w_total > 1:
                    raise ValueError("threshold_method='se' needs a summed sample_weight above 1 "
                                     "(frequency weights: the divisor is sum w - 1)")
                w = self._sw[:, None]
                mean = (w * Y).sum(axis=0) / self._w_total
                spread = np.sqrt((w * (Y - mean) ** 2).sum(axis=0) / (self._w_total - 1))
            return float(150 * -log(self.spreading_factor) * np.linalg.norm(spread))
        raise ValueError("threshold_method not supported. Must be 'se' or 'classical'.")

    def _sync_views(self, refresh_weights: bool) -> None:
        lat = self._lattice
        self.som_ = lat.graph
        self.neurons_ = lat.nodes
        self._distance_matrix = lat.hop_distances()
        if refresh_weights:
            self.weights_ = np.array(lat.W)

    # -- epoch loop (BaseSom.py:387-417) --------------------------------------------------------
    def _grow_som(self, data, y) -> None:
        engine = self._engine()
        lat = self._lattice
        epochs = range(self.n_iter)
        if self.verbose:
            from tqdm import tqdm

            epochs = tqdm(iterable=epochs, unit=" epochs")
        need_assign = self.growth_criterion == "entropy"
        on_targets = self.growth_criterion == "target_error"
        n_classes = 0
        if need_assign:
            if isinstance(data, DeviceSamples):
                # A device subset brought its PARENT's label codes along; this fit has re-coded y
                # (np.unique in fit), and the subset's rows are in the stable bucket order the
                # caller cut y_sub in (y[winners == j]): attach the child's own codes.
                engine.set_labels(y)
            else:
                lo, hi = (0, data.shape[0]) if self._local_input() else self._shard
                engine.set_labels(y[lo:hi])
            n_classes = int(self.classes_.shape[0])
        # The prototypes live in HBM for the whole fit: the first epoch uploads
        # the four start vectors, every later one consumes what the previous one left there; a
        # growth step writes only the inserted rows (and the new hop matrix); the host copy is
        # refreshed at growth steps and at the end.  Backends without resident prototypes (the
        # oracle's CPU stand-in in the tests) get the matrix handed over every epoch.
        # Rows with missing entries: nothing stays resident between masked epochs, whatever the backend can do.
        # The same under metric="manhattan" and metric="cosine": their searches read the prototypes they are handed.
        incomplete = self._incomplete_fit
        manhattan = self._metric_fit == "manhattan"
        cosine = self._metric_fit == "cosine"
        resident = hasattr(engine, "write_weight_rows") and not incomplete and not self._metric_fit
        # growth on the target's error: the targets go next to the rows once; an epoch that leaves its winners in HBM
        # is followed by target_statistics on them, every other epoch hands its winners over
        assign = {}
        if on_targets:
            engine.set_targets(y)
            if not resident:
                assign = {"want_assignments": True}
        on_device = False     # the current prototypes are in HBM, lat.W is stale
        ran = False
        self._growth_epochs = []
        for epoch in epochs:
            self._current_epoch = epoch
            if epoch > self.coarse_training_frac * self.n_iter:
                self._training_phase = "fine"
            self._sync_views(refresh_weights=not on_device)  # hop matrix recomputed only after growth
            w_in = RESIDENT if on_device else self.weights_

            if incomplete:
                res = engine.epoch_masked(w_in, self._distance_matrix, self._calculate_current_sigma(),
                                          self._gamma(), n_classes=n_classes if need_assign else 0, **assign)
            elif manhattan:
                res = engine.epoch_manhattan(w_in, self._distance_matrix, self._calculate_current_sigma(),
                                             self._gamma(), self.centres_layout,
                                             n_classes=n_classes if need_assign else 0, **assign)
            elif cosine:
                res = engine.epoch_cosine(w_in, self._distance_matrix, self._calculate_current_sigma(),
                                          self._gamma(), self.centres_layout,
                                          n_classes=n_classes if need_assign else 0, **assign)
            else:
                res = engine.epoch(w_in, self._distance_matrix, self._calculate_current_sigma(),
                                   self._gamma(), self.centres_layout,
                                   n_classes=n_classes if need_assign else 0,
                                   **({"keep_on_device": True} if resident else {}), **assign)
            ran = True
            if manhattan and not np.isfinite(res.new_weights).all():
                # L1 distances grow with the number of features while gamma = 1 / total variance does not: once
                # gamma d^2 is above 53 ln 2 = 36.7 the sample kernel 1 - sqrt(1 - exp(-gamma d^2)) is 0.0 exactly,
                # and a neuron all of whose rows are that far has the centre 0 / 0 (as in the reference's update)
                raise ValueError(f"metric={self.metric!r} (Manhattan): the update gave prototypes that are not finite in "
                                 f"epoch {epoch}: the sample kernel 1 - sqrt(1 - exp(-d^2 / total variance)) is 0 for "
                                 "every row of a neuron, because squared L1 distances grow with the square of the number of "
                                 "features and the variance only with the number; reduce the features (a projection) or "
                                 "use metric='euclidean'")
            if cosine and not np.isfinite(res.new_weights).all():
                # cosine distances lie in [0, 2] whatever the scale of the data while gamma = 1 / total variance follows
                # it: on data of a tiny total variance the sample kernel is 0.0 for every row of a neuron and its
                # centre is 0 / 0 (as in the reference's update)
                raise ValueError(f"metric={self.metric!r} (cosine): the update gave prototypes that are not finite in "
                                 f"epoch {epoch}: the sample kernel 1 - sqrt(1 - exp(-d^2 / total variance)) is 0 for "
                                 "every row of a neuron, because cosine distances do not scale with the data while "
                                 "the total variance does; rescale X (e.g. to unit total variance) or use "
                                 "metric='euclidean'")
            if resident:
                on_device = True
            else:
                lat.set_weights(res.new_weights)  # like the reference: the graph moves on, the
            if res.change_total < self.convergence_treshold:  # weights_ snapshot stays (Q3)
                self.converged_ = True
            if need_assign:  # label entropy per neuron from the (M, n_classes) histogram
                lat.set_errors(np.array([scipy.stats.entropy(row[: np.flatnonzero(row).max() + 1]
                                                             if row.any() else row[:0], base=2)
                                         for row in res.class_hist]))
            elif on_targets:  # err_j = sum over the unit's rows of w_i ||y_i - mean_j||_2
                lat.set_errors(np.asarray(engine.target_statistics(None if resident else res.winners, len(lat),
                                                                   want_err=True)[3]))
            else:
                lat.set_errors(res.errors)

            if self.converged_ and self._training_phase == "fine":
                break
            if (self._training_phase == "coarse" and len(self.neurons_) < self.max_neurons
                    and epoch % self.convergence_iter == self.convergence_iter - 1):
                lat.distribute_errors(self.growing_threshold_)
                if on_device:
                    if not lat.will_grow(self.growing_threshold_):
                        continue
                    lat.set_weights(engine.get_weights(0))   # growth extrapolates from W'
                    m_before = len(lat)
                    lat.grow(self.growing_threshold_, epoch)
                    self._growth_epochs.append(epoch)
                    for i in lat.pop_overwritten():           # occupied positions (rare)
                        engine.write_weight_rows(i, lat.W[i])
                    if len(lat) > m_before:                   # the inserted rows only
                        engine.write_weight_rows(m_before, lat.W[m_before:])
                else:
                    lat.grow(self.growing_threshold_, epoch)
        if on_device and ran:
            self.weights_ = engine.get_weights(1)   # the snapshot the last epoch consumed (Q3)
            lat.set_weights(engine.get_weights(0))
        if incomplete and ran:
            # (the statistics behind the loop are taken on the last update: the reference has no fit on incomplete
            #  rows whose snapshot of the last epoch's input (Q3) there would be to reproduce)
            self._sync_views(refresh_weights=True)
        if hasattr(engine, "traffic"):
            self._training_traffic = engine.traffic()   # what crossed PCIe during the epoch loop
        lat.write_attributes()

    def _gamma(self) -> float:
        return float(self._total_variance ** -1)

    def _calculate_current_sigma(self) -> float:
        return schedule.current_sigma(
            epoch=self._current_epoch, n_neurons=len(self._lattice), n_iter=self.n_iter,
            phase=self._training_phase, decay_function=self.decay_function,
            learning_rate=self.learning_rate, coarse_training_frac=self.coarse_training_frac,
            sigma_start=self.sigma_start, sigma_end=self.sigma_end)

    def _entropy_errors(self, winners, y):
        out = np.zeros(len(self.neurons_))
        for j in range(len(self.neurons_)):
            out[j] = scipy.stats.entropy(np.bincount(y[winners == j]), base=2)
        return out

    # ------------------------------------------------------------------------------------------
    # the reference's four hot-path methods, same names and argument meaning
    # ------------------------------------------------------------------------------------------
    def _is_resident(self, data) -> bool:
        return getattr(self, "_resident", None) is data

    def _gather_rows(self, local):
        """Concatenate per-rank row shards (identity for one process, and when every rank was
        given only its own rows): ONE padded tensor all_gather, no pickling."""
        rank, world = dist_info()
        if world == 1 or self._local_input():
            return local
        import torch
        import torch.distributed as td

        n = self._n_total
        bounds = [shard_bounds(n, r, world) for r in range(world)]
        longest = max(hi - lo for lo, hi in bounds)
        local = np.ascontiguousarray(local)
        pad = np.zeros((longest,) + local.shape[1:], dtype=local.dtype)
        pad[: local.shape[0]] = local
        mine = torch.from_numpy(pad)
        if td.get_backend() == "nccl":
            mine = mine.cuda()
        parts = [torch.empty_like(mine) for _ in range(world)]
        td.all_gather(parts, mine)
        return np.concatenate([p.cpu().numpy()[: hi - lo] for p, (lo, hi) in zip(parts, bounds)],
                              axis=0)

    def _resident_winners(self, data) -> np.ndarray:
        """The winners of the resident samples on the host; for rows that live in HBM only, without their
        distances' trip across PCIe where the backend can."""
        engine = self._engine()
        if isinstance(data, DeviceSamples) and hasattr(engine, "resident_winners"):
            return engine.resident_winners(self.weights_)
        return self._get_winning_neurons(data, n_bmu=1)[1]

    def _get_winning_neurons(self, data, n_bmu: int):
        """Distances and indices of the n_bmu best matching units (BaseSom.py:446-464)."""
        engine = self._engine()
        if self._is_resident(data):
            dist, idx = engine.bmu(self.weights_, n_bmu)   # (a fit under metric="manhattan" / "cosine": that search, set_metric)
            return self._gather_rows(dist), self._gather_rows(idx)
        kind = self._search_metric()
        if kind:
            self._check_metric_query(kind, data)
            return getattr(engine, f"bmu_{kind}")(self.weights_, n_bmu, data)
        if self._accepts_nan() and isinstance(data, np.ndarray):
            rows = self._incomplete_rows(data)
            if rows.size:
                return self._winning_neurons_with_holes(engine, data, rows, n_bmu)
        return engine.bmu(self.weights_, n_bmu, X=data)

    # ------------------------------------------------------------------------------------------
    # queries on rows with missing entries (missing_values="nan")
    # ------------------------------------------------------------------------------------------
    def _accepts_nan(self) -> bool:
        """Whether the queries take NaN as "missing" (``missing_values="nan"``, or ``"nan-fit"``, which opens ``fit``
        as well); None: NaN is refused."""
        if self.missing_values is None:
            return False
        if isinstance(self.missing_values, str) and self.missing_values in ("nan", "nan-fit"):
            return True
        raise ValueError(f"missing_values must be None, 'nan' or 'nan-fit', got {self.missing_values!r}")

    def _check_query(self, X, accept_sparse="csr"):
        """check_array of a query: float32 kept, anything else float64; with ``missing_values="nan"`` NaN passes in
        dense X (infinities never do, and a NaN among the stored entries of sparse X is refused as ever)."""
        if is_device_array(X):
            return self._check_device_array(X, fit=False)
        if not self._accepts_nan():
            return check_array(X, dtype=[np.float64, np.float32], accept_sparse=accept_sparse)
        X = check_array(X, dtype=[np.float64, np.float32], accept_sparse=accept_sparse, **self._finite_kw("allow-nan"))
        if is_sparse(X):
            from sklearn.utils import assert_all_finite

            assert_all_finite(X.data)
        return X

    @staticmethod
    def _incomplete_rows(X) -> np.ndarray:
        """Indices of the rows of dense X with a NaN; a row with nothing but NaN is refused here, on the host."""
        holes = np.isnan(X)
        rows = np.flatnonzero(holes.any(axis=1))
        if rows.size:
            empty = holes[rows].all(axis=1)
            if empty.any():
                raise ValueError(f"row {int(rows[np.argmax(empty)])} of X has no observed entry: a row needs at "
                                 "least one value that is not NaN")
        return rows

    def _winning_neurons_with_holes(self, engine, data, rows, n_bmu):
        """The rows `rows` of data go through the search over their observed entries (``bmu_masked``), the complete
        rows through ``bmu`` as ever -- their results are those of a call on just them -- and both are put back in
        row order."""
        n = data.shape[0]
        shape = (n,) if n_bmu == 1 else (n, n_bmu)
        dist, idx = np.empty(shape, dtype=np.float64), np.empty(shape, dtype=np.int64)
        dist[rows], idx[rows] = engine.bmu_masked(self.weights_, n_bmu, data[rows])
        if rows.size < n:
            complete = np.ones(n, dtype=bool)
            complete[rows] = False
            complete = np.flatnonzero(complete)
            dist[complete], idx[complete] = engine.bmu(self.weights_, n_bmu, X=data[complete])
        return dist, idx

    def prototype_distances(self, X):
        """The distance from every row of X to every prototype: ``(n_samples, n_prototypes)`` float64, entry
        ``[i, j]`` from row ``i`` to ``weights_[j]`` (the order of ``neurons_``) -- the cluster-distance space
        of ``KMeans.transform``.  The arithmetic is that of the best-matching-unit search, bit for bit, so a row's
        smallest entry is its distance to the unit ``predict`` names; there is no float32 rounding.  X is what
        ``predict`` takes: a dense array (the result is a NumPy array), a device array (a float64 tensor on X's
        device that the GPU writes itself; X and the result never touch the host), scipy sparse rows (the result
        of the dense call on ``X.toarray()``), and with ``missing_values`` set rows with NaN, whose entries are
        ``sqrt(d / n_obs * sum over the observed (x_k - w_k)^2)``.  Under ``metric="manhattan"`` the entries are
        ``sum_k |x_k - w_k|`` in float64, under ``metric="cosine"`` ``1 - <x, w> / (|x| |w|)`` clamped to [0, 2]
        (dense X and tensors only).  Only this map's prototypes are used (not the
        child maps of vertical growth); the call is local to the process."""
        check_is_fitted(self)
        W = self.weights_
        if not is_device_array(X) and not is_sparse(X) and np.ndim(X) == 2 and np.shape(X)[0] == 0:
            X = check_array(X, dtype=[np.float64, np.float32], ensure_min_samples=0)   # (no rows: no launch)
        else:
            X = self._check_query(X)
        if X.shape[1] != self.n_features_in_:
            raise ValueError(f"X has {X.shape[1]} features, but {type(self).__name__} is expecting "
                             f"{self.n_features_in_} features as input")
        if X.shape[0] == 0:
            return np.empty((0, len(W)), dtype=np.float64)
        engine = self._engine()
        kind = self._search_metric()
        if kind:   # sum_k |x_k - w_k| / the cosine distance, the arithmetic of that search bit for bit
            self._check_metric_query(kind, X)
            return getattr(engine, f"distances_{kind}")(W, X)
        if self._accepts_nan() and isinstance(X, np.ndarray):
            rows = self._incomplete_rows(X)
            if rows.size:   # split and scatter as _winning_neurons_with_holes
                out = np.empty((X.shape[0], len(W)), dtype=np.float64)
                out[rows] = engine.distances_masked(W, X[rows])
                if rows.size < X.shape[0]:
                    complete = np.ones(X.shape[0], dtype=bool)
                    complete[rows] = False
                    complete = np.flatnonzero(complete)
                    out[complete] = engine.distances(W, X[complete])
                return out
        return engine.distances(W, X)

    def kneighbors(self, X, n_neighbors=5, return_distance=True):
        """The ``n_neighbors`` nearest prototypes of every row of X: ``(dist, idx)``, or ``idx`` alone with
        ``return_distance=False``, both ``(n_samples, n_neighbors)``, float64 and int64 (indices into ``weights_``,
        the order of ``neurons_``) -- ``NearestNeighbors.kneighbors`` on the prototypes.

        Row ``i`` holds the prototypes with the smallest ``(r_ij, j)`` in lexicographic order, ascending, where
        ``r_ij = max((|x_i|^2 + (-2 <x_i, w_j>)) + |w_j|^2, 0)`` is the squared value of the best-matching-unit
        search's own arithmetic; ``dist = sqrt(r)`` is taken after the selection and there is no float32 rounding.
        The selection is on ``r``: of two different ``r`` under one square root the smaller comes first, whatever
        the indices; equal ``r`` go by the lower index.  So ``idx[:, :2]`` are the two units of the topographic
        error, ``idx[:, 0]`` equals ``predict(X)``, and ``dist[i, t] == prototype_distances(X)[i, idx[i, t]]`` bit
        for bit.  A pair whose ``r`` is not below +inf is never reported; slots left unfilled hold ``(inf, -1)``.
        With ``missing_values`` set, rows with NaN are ordered by ``d / n_obs * sum over the observed
        (x_k - w_k)^2`` with the same tie rule.  Under ``metric="manhattan"`` the order is on
        ``(sum_k |x_k - w_k|, j)`` and ``dist`` is that sum, under ``metric="cosine"`` likewise with the cosine distance:
        no square root is taken (dense X and tensors only).

        ``1 <= n_neighbors <= min(len(weights_), 32)``; the selection runs on the GPU for every such value, and
        above 32 ``prototype_distances(X)`` and a sort of one's own is the route.  X is what ``predict`` takes: a
        dense array (NumPy results), a device array (tensors on X's device that the GPU writes itself; X and the
        results never touch the host), scipy sparse rows, rows with NaN under ``missing_values``.  The N x M
        matrix is never held: squared distances live one slab of rows at a time on the device.  Only this map's
        prototypes are used (not the child maps of vertical growth); the call is local to the process."""
        check_is_fitted(self)
        W = self.weights_
        if isinstance(n_neighbors, (bool, np.bool_)) or not isinstance(n_neighbors, (numbers.Integral, np.integer)):
            raise ValueError("n_neighbors does not take %s value, enter integer value" % type(n_neighbors))
        k = int(n_neighbors)
        if k <= 0:
            raise ValueError("Expected n_neighbors > 0. Got %d" % k)
        if not is_device_array(X) and not is_sparse(X) and np.ndim(X) == 2 and np.shape(X)[0] == 0:
            X = check_array(X, dtype=[np.float64, np.float32], ensure_min_samples=0)   # (no rows: no launch)
        else:
            X = self._check_query(X)
        if X.shape[1] != self.n_features_in_:
            raise ValueError(f"X has {X.shape[1]} features, but {type(self).__name__} is expecting "
                             f"{self.n_features_in_} features as input")
        if k > len(W):
            raise ValueError("Expected n_neighbors <= n_samples_fit, but n_neighbors = %d, n_samples_fit = %d "
                             "(the prototypes), n_samples = %d" % (k, len(W), X.shape[0]))
        if k > MAX_NEIGHBORS:
            raise ValueError(f"n_neighbors = {k} is above the {MAX_NEIGHBORS} the selection on the GPU keeps per row: "
                             "use prototype_distances(X) and sort its rows")
        if X.shape[0] == 0:
            dist, idx = np.empty((0, k), dtype=np.float64), np.empty((0, k), dtype=np.int64)
            return (dist, idx) if return_distance else idx
        engine = self._engine()
        dist = idx = None
        kind = self._search_metric()
        if kind:   # the k smallest (sum_k |x_k - w_k|, j) / (cosine distance, j): no square root behind the selection
            self._check_metric_query(kind, X)
            dist, idx = getattr(engine, f"kneighbors_{kind}")(W, k, X)
            return (dist, idx) if return_distance else idx
        if self._accepts_nan() and isinstance(X, np.ndarray):
            rows = self._incomplete_rows(X)
            if rows.size:   # split and scatter as _winning_neurons_with_holes
                dist, idx = np.empty((X.shape[0], k), dtype=np.float64), np.empty((X.shape[0], k), dtype=np.int64)
                dist[rows], idx[rows] = engine.kneighbors_masked(W, k, X[rows])
                if rows.size < X.shape[0]:
                    complete = np.ones(X.shape[0], dtype=bool)
                    complete[rows] = False
                    complete = np.flatnonzero(complete)
                    dist[complete], idx[complete] = engine.kneighbors(W, k, X[complete])
        if idx is None:
            dist, idx = engine.kneighbors(W, k, X)
        return (dist, idx) if return_distance else idx

    def impute(self, X) -> np.ndarray:
        """A copy of X (float32 kept, anything else float64) with every NaN replaced by that entry of the row's
        best matching prototype, the nearest one over the row's observed entries.  Observed entries and complete
        rows come back bit for bit, X itself is never written.  Needs ``missing_values="nan"``; dense X; only this
        map's prototypes are used (not the child maps of vertical growth)."""
        check_is_fitted(self)
        if not self._accepts_nan():
            raise ValueError("impute needs missing_values='nan' (or 'nan-fit')")
        return self._impute_checked(self._check_query(X, accept_sparse=False), copy=True)

    def _impute_checked(self, X, copy=False):
        rows = self._incomplete_rows(X)
        if copy or rows.size:
            X = X.copy()
        if rows.size:
            X[rows] = self._engine().bmu_masked(self.weights_, 1, X[rows], want_filled=True)[2]
        return X

    def _complete_query(self, X):
        """A validated query for the coder: rows with NaN are completed by ``impute`` (the sparse code works on
        normalised rows and has no meaning for a hole)."""
        if self._accepts_nan() and isinstance(X, np.ndarray):
            return self._impute_checked(X)
        return X

    def _calculate_exp_similarity(self, distances):
        """Per-sample weight 1 - sqrt(1 - exp(-gamma d^2)) (BaseSom.py:533-538)."""
        return self._engine().exp_similarity(distances, self._gamma())

    def _update_weights(self, sample_weights, winners, data) -> None:
        """Batch update of all prototypes (BaseSom.py:470-523) on the resident samples."""
        if not self._is_resident(data):
            self._load_resident(data)
        lo, hi = (0, len(winners)) if self._local_input() else self._shard
        winners = np.asarray(winners)[lo:hi]
        Wn, chg, _, _ = self._engine().update(
            self.weights_, self._distance_matrix, self._calculate_current_sigma(),
            np.asarray(sample_weights)[lo:hi], winners, np.zeros(len(winners)),
            self.centres_layout)
        self._lattice.set_weights(Wn)
        if chg < self.convergence_treshold:
            self.converged_ = True
        self._lattice.write_attributes()

    def _write_accumulative_error(self, winners, y, distances) -> None:
        """Per-neuron error = sum of BMU distances, or label entropy (BaseSom.py:541-561)."""
        if self.growth_criterion == "entropy":
            errors = self._entropy_errors(np.asarray(winners), y)
        else:
            errors = np.bincount(winners, weights=distances, minlength=len(self.neurons_))
        self._lattice.set_errors(errors)
        self._lattice.write_attributes()

    # ------------------------------------------------------------------------------------------
    # post-fit statistics (BaseSom.py:181-235, 904-953)
    # ------------------------------------------------------------------------------------------
    def calculate_quantization_error(self, X) -> float:
        """Average distance from each sample to its nearest prototype."""
        check_is_fitted(self)
        if self._is_resident(X):  # during fit: a device reduction, distances never leave HBM
            return self._engine().quantization_error(self.weights_)
        X = self._check_query(X)
        distances, _ = self._get_winning_neurons(X, n_bmu=1)
        # (a device array's distances go to the host for the mean: NumPy's pairwise sum, bit for bit -- N x 8 bytes)
        return float(np.mean(self._host(distances)))

    def _neighborhood_factors(self, sigma) -> np.ndarray:
        """``H = exp(-(hop^2 / (2 sigma^2)))`` on the host, hop the hop distances of the fitted lattice in the order of
        ``neurons_`` (``inf`` between disconnected components: h = 0).  ``sigma=None``: the bandwidth of the last
        training epoch."""
        if sigma is None:
            sigma = self._calculate_current_sigma()
        elif isinstance(sigma, (bool, np.bool_)) or not isinstance(sigma, (numbers.Real, np.floating, np.integer)):
            raise ValueError(f"sigma must be None or a finite float > 0, got {sigma!r}")
        sigma = float(sigma)
        if not (np.isfinite(sigma) and sigma > 0.0):
            raise ValueError(f"sigma must be None or a finite float > 0, got {sigma!r}")
        hop = self._distance_matrix   # (of the map as it is after the dead units were removed: _sync_views)
        if hop.shape != (len(self.weights_),) * 2:
            hop = self._lattice.hop_distances()
        return np.exp(-(hop ** 2 / (2 * sigma ** 2)))

    def sample_distortion(self, X, sigma=None):
        """The SOM distortion measure row by row: ``(e, bmu)``, both ``(n_samples,)``, float64 and int64, with
        ``e_i = sum_j h(b_i, j) * ||x_i - w_j||^2``, ``b_i`` the best matching unit of row ``i`` (``predict``'s
        unit for ``SomVQ``, an index into ``weights_``) and ``h(b, j) = exp(-(hop(b, j)^2 / (2 sigma^2)))`` over the
        hop distances of the lattice -- the quantity the batch rule descends on (Kohonen's energy with a fixed
        neighbourhood; SOM Toolbox ``som_distortion``).  Large ``e`` at small quantization error marks rows whose
        unit's lattice neighbours are far away in the input space: where the map is folded.

        ``sigma=None`` is the bandwidth of the last training epoch, otherwise a finite float > 0.  The squared
        distances are those of the best-matching-unit search's own arithmetic, ``r_ij = max((|x_i|^2 + (-2 <x_i,
        w_j>)) + |w_j|^2, 0)``, without float32 rounding, and the order of the sum is fixed (64 strided partials of
        rounded products, then six xor rounds), so the result does not depend on chunks, slabs or where X lives.
        H is computed on the host and uploaded once per call (8 M^2 bytes); the N x M matrix is never held.

        X is what ``kneighbors`` takes under the Euclidean metric: a dense array (NumPy results), a tensor on the
        estimator's GPU (tensors on X's device that the GPU writes itself; X never touches the host), scipy sparse
        rows (the dense call's result on ``X.toarray()``).  Refused with a ``ValueError``: ``metric="manhattan"`` /
        ``"cosine"`` (the measure is defined on squared Euclidean distances), rows with NaN (also under
        ``missing_values``: impute them first), a feature-count mismatch.  Only this map's prototypes are used (not
        the child maps of vertical growth); the call is local to the process."""
        check_is_fitted(self)
        kind = self._search_metric()
        if kind:
            self._refuse_metric(kind, "sample_distortion / calculate_distortion",
                                "the measure is defined on squared Euclidean distances")
        H = self._neighborhood_factors(sigma)
        if not is_device_array(X) and not is_sparse(X) and np.ndim(X) == 2 and np.shape(X)[0] == 0:
            X = check_array(X, dtype=[np.float64, np.float32], ensure_min_samples=0)   # (no rows: no launch)
        else:
            X = self._check_query(X)
        if X.shape[1] != self.n_features_in_:
            raise ValueError(f"X has {X.shape[1]} features, but {type(self).__name__} is expecting "
                             f"{self.n_features_in_} features as input")
        if isinstance(X, np.ndarray) and np.isnan(X).any():   # (passed _check_query: missing_values is set)
            raise ValueError(f"X holds NaN: the distortion measure is not defined on rows with missing entries "
                             f"(missing_values={self.missing_values!r}); impute them first (impute(X))")
        if X.shape[0] == 0:
            return np.empty(0, dtype=np.float64), np.empty(0, dtype=np.int64)
        return self._engine().neighborhood_energy(self.weights_, H, X)

    def calculate_distortion(self, X, sigma=None) -> float:
        """The SOM distortion measure of X: the mean of ``sample_distortion(X, sigma)[0]``.  The per-row values come
        to the host (8 bytes per row) and NumPy sums them, so a host array and a tensor holding the same rows give
        the same float."""
        e, _ = self.sample_distortion(X, sigma)
        if e.shape[0] == 0:
            check_array(X, dtype=[np.float64, np.float32])   # (no rows: refused in check_array's words, as a mean is)
        return float(np.sum(self._host(e))) / e.shape[0]

    def prototype_exemplars(self, X, n_exemplars=1, own_cell=False, return_distance=True):
        """The ``n_exemplars`` nearest rows of X to every prototype: ``(dist, idx)``, or ``idx`` alone with
        ``return_distance=False``, both ``(len(weights_), n_exemplars)``, float64 and int64 (row numbers of X) -- the
        records that stand for a unit: its medoid, the exemplar images of a map, the documents of a cell;
        ``pairwise_distances_argmin_min(weights_, X)`` for ``n_exemplars=1``.

        Row ``j`` holds the rows of X with the smallest ``(r_ij, i)`` in lexicographic order, ascending, where
        ``r_ij = max((|x_i|^2 + (-2 <x_i, w_j>)) + |w_j|^2, 0)`` is the squared value of the best-matching-unit
        search's own arithmetic, the one ``kneighbors`` selects on; ``dist = sqrt(r)`` is taken after the selection.
        Equal ``r`` go by the lower row number, and of two different ``r`` under one square root the smaller comes
        first.  A pair whose ``r`` is not below +inf is never reported; slots left unfilled hold ``(inf, -1)``: with
        fewer rows than ``n_exemplars``, or with an empty cell under ``own_cell``.  Invariants:

        * ``dist[j, t] == prototype_distances(X)[idx[j, t], j]`` bit for bit;
        * ``own_cell=True``: row ``i`` is a candidate for unit ``j`` only if ``j`` is the row's best matching unit,
          the index of the smallest ``(r_ij, j)`` -- what ``SomVQ.predict`` and ``kneighbors(X, 1)`` name (a row
          without any ``r`` below +inf belongs to no cell).  Every filled slot then satisfies
          ``kneighbors(X[idx[j, t]], 1)[1] == j``, row ``j`` has ``min(n_exemplars, rows whose unit is j)`` filled
          slots, and ``dist[j, 0]`` is the smallest distance in the cell;
        * ``(r, i)`` is a total order, so the result does not depend on chunks, slabs or where X lives: a host
          array, a tensor and CSR rows of the same data give the same bits.

        ``1 <= n_exemplars <= 32``; it may exceed the number of rows, and above 32 ``prototype_distances(X)`` and a
        sort of its columns is the route.  X is what ``kneighbors`` takes under the Euclidean metric: a dense array
        (NumPy results; ``len(weights_) * n_exemplars * 16`` bytes come down, once, at the end of the call), a tensor
        on the estimator's GPU (tensors on X's device that the GPU writes itself; X never touches the host), scipy
        sparse rows (the dense call's result on ``X.toarray()``).  X without rows gives all ``(inf, -1)`` without a
        launch.  The N x M matrix is never held: squared distances live one slab of rows at a time on the device
        and a selection down its columns folds them into the result.  Refused with a ``ValueError``:
        ``metric="manhattan"`` / ``"cosine"``, rows with NaN (also under ``missing_values``: impute them first), a
        feature-count mismatch.  Only this map's prototypes are used (not the child maps of vertical growth); the
        call is local to the process."""
        check_is_fitted(self)
        if isinstance(n_exemplars, (bool, np.bool_)) or not isinstance(n_exemplars, (numbers.Integral, np.integer)):
            raise ValueError("n_exemplars does not take %s value, enter integer value" % type(n_exemplars))
        k = int(n_exemplars)
        if k <= 0:
            raise ValueError("Expected n_exemplars > 0. Got %d" % k)
        if k > MAX_NEIGHBORS:
            raise ValueError(f"n_exemplars = {k} is above the {MAX_NEIGHBORS} the selection on the GPU keeps per "
                             "prototype: use prototype_distances(X) and sort its columns")
        kind = self._search_metric()
        if kind:
            self._refuse_metric(kind, "prototype_exemplars",
                                "the selection runs on the squared Euclidean distances of the search")
        if not is_device_array(X) and not is_sparse(X) and np.ndim(X) == 2 and np.shape(X)[0] == 0:
            X = check_array(X, dtype=[np.float64, np.float32], ensure_min_samples=0)   # (no rows: no launch)
        else:
            X = self._check_query(X)
        if X.shape[1] != self.n_features_in_:
            raise ValueError(f"X has {X.shape[1]} features, but {type(self).__name__} is expecting "
                             f"{self.n_features_in_} features as input")
        if isinstance(X, np.ndarray) and np.isnan(X).any():   # (passed _check_query: missing_values is set)
            raise ValueError(f"X holds NaN: the exemplars of a unit are not defined on rows with missing entries "
                             f"(missing_values={self.missing_values!r}); impute them first (impute(X))")
        M = len(self.weights_)
        if X.shape[0] == 0 and not is_device_array(X):
            dist, idx = np.full((M, k), np.inf), np.full((M, k), -1, dtype=np.int64)
        else:
            dist, idx = self._engine().exemplars(self.weights_, k, X, own_cell=bool(own_cell))
        return (dist, idx) if return_distance else idx

    # ------------------------------------------------------------------------------------------
    # nearest stored rows through the map: an inverted-file index over the units
    # ------------------------------------------------------------------------------------------
    _index = None   # (backend, its resident_serial, weights_) of the last index_rows

    def _check_index_input(self, X, what: str):
        """The refusals index_rows and row_neighbors share, in front of any upload -> the validated rows"""
        kind = self._search_metric()
        if kind:
            self._refuse_metric(kind, what, "rows are compared by the squared Euclidean distance; use metric='euclidean'")
        if self.sharded_input or dist_info()[1] > 1:
            raise ValueError(f"{what} takes one process: no sharded_input, no process group of more than one rank")
        if is_sparse(X) or getattr(X, "is_sparse", False):
            raise TypeError(f"{what} takes dense rows: pass X.toarray() (the stored rows are scanned as dense rows)")
        if self.n_features_in_ > MAX_SCAN_FEATURES:
            raise ValueError(f"{what} scans rows of at most {MAX_SCAN_FEATURES} features (the widened query lives in "
                             f"64 KiB of LDS), this map has {self.n_features_in_}: reduce the features first")
        if not is_device_array(X) and np.ndim(X) == 2 and np.shape(X)[0] == 0 and what == "row_neighbors":
            X = check_array(X, dtype=[np.float64, np.float32], ensure_min_samples=0)   # (no rows: no launch)
        else:
            X = self._check_query(X, accept_sparse=False)
        if X.shape[1] != self.n_features_in_:
            raise ValueError(f"X has {X.shape[1]} features, but {type(self).__name__} is expecting "
                             f"{self.n_features_in_} features as input")
        if isinstance(X, np.ndarray) and np.isnan(X).any():   # (passed _check_query: missing_values is set)
            raise ValueError(f"X holds NaN: {what} is not defined on rows with missing entries "
                             f"(missing_values={self.missing_values!r}); impute them first (impute(X))")
        return X

    def index_rows(self, X):
        """File the rows of X under their best matching units and keep them in HBM: the index ``row_neighbors``
        searches.  X is made resident the way ``fit`` does it -- a host array is uploaded once, a tensor on the
        estimator's GPU is read in place when it is float32 / float64 with contiguous rows of a multiple of 16
        features (do not write to it while the index is in use), else pad-copied on the device -- and bucketed by
        unit on the GPU.  Sets ``index_counts_``, the rows per unit as ``(len(weights_),)`` int64, and
        ``n_indexed_``; the map and everything ``fit`` set stay as they are.  The index lives until the next
        ``index_rows`` or ``fit``, and is not pickled.  Refused: sparse X (``TypeError``), ``metric`` other than the
        Euclidean one, NaN (also under ``missing_values``), more than one rank or ``sharded_input``, a tensor on
        another GPU, more than 8192 features."""
        check_is_fitted(self)
        X = self._check_index_input(X, "index_rows")
        engine = self._engine()
        self._index = None
        if is_device_array(X):
            if not hasattr(engine, "load_device"):
                raise TypeError(f"the {engine.name} backend takes host arrays only: pass X.cpu().numpy()")
            engine.load_device(X)
        else:
            engine.load(X)
        counts, _ = engine.partition(self.weights_)
        self.index_counts_ = np.asarray(counts, dtype=np.int64)
        self.n_indexed_ = int(X.shape[0])
        self._index = (engine, engine.resident_serial, self.weights_)
        return self

    def row_neighbors(self, Q, n_neighbors=5, n_probe=8, return_distance=True):
        """The ``n_neighbors`` nearest indexed rows of every row of Q, looked for under its ``n_probe`` nearest units
        only: ``(dist, idx)``, or ``idx`` alone with ``return_distance=False``, both ``(len(Q), n_neighbors)``,
        float64 and int64 (row numbers of the X given to ``index_rows``) -- WEBSOM-style retrieval, the map as an
        inverted-file index.

        The units of row q are ``kneighbors(Q, n_probe)``'s indices (a ``-1`` slot is skipped); its candidates are
        the indexed rows ``i`` whose unit, ``predict(X)[i]``, is among them.  ``rho(i, q)`` is the direct-form
        squared distance in float64 (float32 values widened exactly) in a fixed order, ``backend.rho_rows`` bit for
        bit.  Row q of the result holds the candidates with the smallest ``(rho, i)`` in lexicographic order,
        ascending; ``dist = sqrt(rho)`` is taken after the selection; only ``rho < +inf`` is listed and unfilled
        slots hold ``(inf, -1)``.  ``(rho, i)`` is a total order: the result does not depend on chunks, on the order
        of rows inside a cell or on where Q lives.  With ``n_probe = len(weights_)`` the search is exact.

        ``1 <= n_neighbors <= 32``, ``1 <= n_probe <= min(len(weights_), 32)``.  Q is a dense host array (NumPy
        results; ``len(Q) * n_neighbors * 16`` bytes come down) or a tensor on the estimator's GPU (tensors on its
        device that the GPU writes itself; nothing of Q or the results crosses PCIe).  Refused with a
        ``ValueError`` (sparse Q: ``TypeError``): no index (``index_rows`` not called, a later ``fit``, a pickle
        round trip, the backend's resident rows replaced since), and everything ``index_rows`` refuses."""
        check_is_fitted(self)
        for name, v in (("n_neighbors", n_neighbors), ("n_probe", n_probe)):
            if isinstance(v, (bool, np.bool_)) or not isinstance(v, (numbers.Integral, np.integer)):
                raise ValueError("%s does not take %s value, enter integer value" % (name, type(v)))
            if int(v) <= 0:
                raise ValueError("Expected %s > 0. Got %d" % (name, int(v)))
        k, n_probe = int(n_neighbors), int(n_probe)
        M = len(self.weights_)
        if k > MAX_NEIGHBORS:
            raise ValueError(f"n_neighbors = {k} is above the {MAX_NEIGHBORS} the selection on the GPU keeps per row")
        if n_probe > M:
            raise ValueError("Expected n_probe <= n_samples_fit, but n_probe = %d, n_samples_fit = %d (the prototypes)"
                             % (n_probe, M))
        if n_probe > MAX_NEIGHBORS:
            raise ValueError(f"n_probe = {n_probe} is above the {MAX_NEIGHBORS} units a row can probe")
        Q = self._check_index_input(Q, "row_neighbors")
        index = self._index
        if index is None:
            raise ValueError("row_neighbors needs an index: call index_rows(X) first (the index is device state: it is "
                             "dropped by fit and by pickling)")
        engine = self._engine()
        if index[0] is not engine or index[1] != engine.resident_serial or index[2] is not self.weights_:
            raise ValueError("the rows index_rows made resident have been replaced since (or the map has changed): call "
                             "index_rows(X) again")
        if Q.shape[0] == 0 and not is_device_array(Q):
            dist, idx = np.empty((0, k), dtype=np.float64), np.empty((0, k), dtype=np.int64)
        else:
            dist, idx = engine.row_neighbors(self.weights_, k, n_probe, Q)
        return (dist, idx) if return_distance else idx

    @staticmethod
    def _check_radii(radius):
        """-> (the radii as a float64 vector, whether the caller gave a single one) for ``prototype_density``"""
        bad = ValueError(f"radius must be None, a finite real number >= 0 or a 1-D array-like of 1 .. {MAX_RADII} of "
                         f"them, got {radius!r}")
        if isinstance(radius, (bool, np.bool_, str, bytes)):
            raise bad
        try:
            rho = np.asarray(radius)
        except (TypeError, ValueError):
            raise bad from None
        if not (np.issubdtype(rho.dtype, np.floating) or np.issubdtype(rho.dtype, np.integer)) or rho.ndim > 1:
            raise bad
        scalar = rho.ndim == 0
        rho = rho.astype(np.float64).reshape(-1)
        if rho.size == 0:
            raise bad
        if rho.size > MAX_RADII:
            raise ValueError(f"{rho.size} radii are above the {MAX_RADII} the count on the GPU keeps per prototype: "
                             "use several calls, or prototype_distances(X) and counts of one's own")
        if not (np.isfinite(rho).all() and (rho >= 0.0).all()):
            raise bad
        return rho, scalar

    def prototype_density(self, X, radius=None):
        """The data density at the prototypes: ``counts[j]`` is the number of rows of X within ``radius`` of
        prototype ``j``, whatever cell they fell into -- Ultsch's P-matrix, the second half of the U*-matrix, and what
        tells a large U-height across an empty gap from one inside a dense region.  int64, ``(len(weights_),)`` for a
        single radius and ``(len(weights_), len(radius))`` for a 1-D array-like of 1 .. 32 radii, columns in the
        caller's order (any order, duplicates allowed): the whole step-kernel profile in one pass over X, as choosing
        a radius (Ultsch's Pareto radius) needs it.

        ``radius=None`` is the mean of the fitted map's U-matrix, the bandwidth of the per-node ``density`` statistic;
        the value used is kept in ``density_radius_``.  Every radius is finite and ``>= 0``.

        ``counts[j, t] = #{ i : sqrt(r_ij) <= radius[t] }`` with ``r_ij = max((|x_i|^2 + (-2 <x_i, w_j>)) + |w_j|^2,
        0)`` the squared value of the best-matching-unit search's own arithmetic, the one ``kneighbors`` and
        ``prototype_exemplars`` select on.  Invariant, integer for integer: ``counts[:, t] ==
        np.count_nonzero(prototype_distances(X) <= radius[t], axis=0)``.  The comparison runs on the squared values
        against the largest float64 under whose correctly rounded root the radius lies, which is the same condition;
        a pair whose ``r`` is NaN is never counted.  Integer counts do not depend on chunks, slabs or where X lives: a
        host array, a tensor and CSR rows of the same data give the same result.

        X is what ``prototype_exemplars`` takes under the Euclidean metric: a dense array (a NumPy result;
        ``len(weights_) * n_radii * 8`` bytes come down, once), a tensor on the estimator's GPU (an int64 tensor on
        X's device that the GPU writes; nothing of X or the result touches the host), scipy sparse rows (the dense
        call's result on ``X.toarray()``).  X without rows gives zeros without a launch.  The N x M matrix is never
        held.  Refused with a ``ValueError``: ``metric="manhattan"`` / ``"cosine"``, rows with NaN (also under
        ``missing_values``: impute them first), a feature-count mismatch, a bad ``radius``; above 32 radii
        ``prototype_distances(X)`` is the route.  Only this map's prototypes are used (not the child maps of vertical
        growth); the call is local to the process."""
        check_is_fitted(self)
        if radius is None:
            rho, scalar = np.array([float(self._get_u_matrix().mean())]), True
        else:
            rho, scalar = self._check_radii(radius)
        kind = self._search_metric()
        if kind:
            self._refuse_metric(kind, "prototype_density / u_star_matrix",
                                "the count runs on the squared Euclidean distances of the search")
        if not is_device_array(X) and not is_sparse(X) and np.ndim(X) == 2 and np.shape(X)[0] == 0:
            X = check_array(X, dtype=[np.float64, np.float32], ensure_min_samples=0)   # (no rows: no launch)
        else:
            X = self._check_query(X)
        if X.shape[1] != self.n_features_in_:
            raise ValueError(f"X has {X.shape[1]} features, but {type(self).__name__} is expecting "
                             f"{self.n_features_in_} features as input")
        if isinstance(X, np.ndarray) and np.isnan(X).any():   # (passed _check_query: missing_values is set)
            raise ValueError(f"X holds NaN: the density at a prototype is not defined on rows with missing entries "
                             f"(missing_values={self.missing_values!r}); impute them first (impute(X))")
        M = len(self.weights_)
        if X.shape[0] == 0 and not is_device_array(X):
            counts = np.zeros((M, rho.size), dtype=np.int64)
        else:
            counts = self._engine().range_counts(self.weights_, squared_thresholds(rho), X)
        self.density_radius_ = float(rho[0]) if scalar else rho.copy()
        return counts[:, 0] if scalar else counts

    def u_star_matrix(self, X, radius=None) -> np.ndarray:
        """The U*-matrix of Ultsch (2003): the U-matrix damped where the data is dense, an ``(len(weights_),)``
        float64 NumPy array.  ``U* = U * scale`` with U the mean input-space distance from every prototype to its
        lattice neighbours and ``scale_j = (P_j - mean(P)) / (mean(P) - max(P)) + 1``, ``P = prototype_density(X,
        radius)`` (a single radius; ``None``: its default): 1 at the mean density, 0 at the densest unit, above 1 in
        sparse regions; 1 everywhere when ``max(P) == mean(P)``.  Computed on the host from ``len(weights_)`` counts.
        X and the refusals are ``prototype_density``'s."""
        if radius is not None and not self._check_radii(radius)[1]:
            raise ValueError(f"u_star_matrix takes one radius, got {radius!r}")
        P = self._host(self.prototype_density(X, radius)).astype(np.float64)
        U = self._get_u_matrix()
        mean, top = P.mean(), P.max()
        if top == mean:
            return U * np.ones_like(P)
        return U * ((P - mean) / (mean - top) + 1.0)

    # ------------------------------------------------------------------------------------------
    # the map as an isotropic Gaussian mixture (csrc/mixture.hip)
    # ------------------------------------------------------------------------------------------
    def _mixture_query(self, X, what: str):
        """The validated rows of a mixture call and its refusals, on the host before anything is uploaded."""
        check_is_fitted(self)
        kind = self._search_metric()
        if kind:
            self._refuse_metric(kind, what, "the model is Gaussian in the Euclidean distance")
        if not is_device_array(X) and not is_sparse(X) and np.ndim(X) == 2 and np.shape(X)[0] == 0:
            X = check_array(X, dtype=[np.float64, np.float32], ensure_min_samples=0)   # (no rows: no launch)
        else:
            X = self._check_query(X)
        if X.shape[1] != self.n_features_in_:
            raise ValueError(f"X has {X.shape[1]} features, but {type(self).__name__} is expecting "
                             f"{self.n_features_in_} features as input")
        if isinstance(X, np.ndarray) and np.isnan(X).any():   # (passed _check_query: missing_values is set)
            raise ValueError(f"X holds NaN: the mixture density is not defined on rows with missing entries "
                             f"(missing_values={self.missing_values!r}); impute them first (impute(X))")
        return X

    @staticmethod
    def _check_bandwidth(bandwidth) -> float:
        if isinstance(bandwidth, (bool, np.bool_)) or not isinstance(bandwidth, (numbers.Real, np.floating, np.integer)):
            raise ValueError(f"bandwidth must be None or a finite float > 0, got {bandwidth!r}")
        h = float(bandwidth)
        if not (np.isfinite(h) and h > 0.0 and 0.0 < 2.0 * h * h < np.inf and np.isfinite(1.0 / (2.0 * h * h))):   # (c finite)
            raise ValueError(f"bandwidth must be None or a finite float > 0, got {bandwidth!r}")
        return h

    def _mixture_params(self, bandwidth, priors):
        """-> (log-priors (M,) float64 with -inf for a unit without mass, c = 1 / (2 h^2), h): the arguments, or for
        each that is None the attribute ``fit_mixture`` set"""
        M = len(self.weights_)
        if bandwidth is None:
            if not hasattr(self, "mixture_bandwidth_"):
                raise ValueError("no bandwidth: call fit_mixture(X) first, or pass bandwidth")
            h = float(self.mixture_bandwidth_)
        else:
            h = self._check_bandwidth(bandwidth)
        if priors is None:
            if not hasattr(self, "mixture_priors_"):
                raise ValueError("no priors: call fit_mixture(X) first, or pass priors (an array, or 'uniform')")
            p = np.asarray(self.mixture_priors_, dtype=np.float64)
            if p.shape != (M,):
                raise ValueError(f"mixture_priors_ holds {p.shape[0]} shares, the map has {M} prototypes: call "
                                 "fit_mixture(X) again")
        elif isinstance(priors, str):
            if priors != "uniform":
                raise ValueError(f"priors must be None, 'uniform' or an array-like of shape ({M},), got {priors!r}")
            p = np.full(M, 1.0 / M)
        else:
            try:
                p = np.asarray(priors, dtype=np.float64)
            except (TypeError, ValueError):
                raise ValueError(f"priors must be None, 'uniform' or an array-like of shape ({M},), "
                                 f"got {priors!r}") from None
            if p.shape != (M,):
                raise ValueError(f"priors must be None, 'uniform' or an array-like of shape ({M},), got shape {p.shape}")
            if not (np.isfinite(p).all() and (p >= 0.0).all()):
                raise ValueError("priors must be finite and non-negative")
            if abs(fsum(p.tolist()) - 1.0) > 1e-9:
                raise ValueError(f"priors must sum to 1 within 1e-9, got a sum of {fsum(p.tolist())!r}")
        with np.errstate(divide="ignore"):
            return np.log(p), 1.0 / (2.0 * h * h), h

    def fit_mixture(self, X, bandwidth=None):
        """Read the fitted map as an isotropic Gaussian mixture of X and return ``self``: the prototypes are the
        centres, ``mixture_priors_`` (``(len(weights_),)`` float64) the shares of the rows of X per best matching unit
        -- zeros allowed: a unit without mass -- and ``mixture_bandwidth_`` the one standard deviation ``h`` of every
        component.  This is the reduced-set density estimate: a kernel density estimate on the prototypes, weighted by
        their hits.

        ``bandwidth=None``: ``h^2 = fsum_i(dist_i^2) / (n d)`` with ``dist`` the ``kneighbors(X, 1)`` distances, the
        maximum-likelihood variance under hard assignments; ``math.fsum`` makes it independent of the order, so a host
        array, a tensor and CSR rows of the same data give the same float.  ``h^2 == 0`` (every row sits on a
        prototype) or a non-finite value is a ``ValueError``.  Otherwise a finite float > 0.  ``2 n x 8`` bytes come to
        the host.  The map itself, and everything ``fit`` set, is left as it is.  X and the refusals are
        ``score_samples``'s; X needs at least one row."""
        X = self._mixture_query(X, "fit_mixture")
        n, M = X.shape[0], len(self.weights_)
        if n == 0:
            check_array(X, dtype=[np.float64, np.float32])   # (no rows: refused in check_array's words)
        h = None if bandwidth is None else self._check_bandwidth(bandwidth)
        dist, idx = self._engine().kneighbors(self.weights_, 1, X)
        dist, idx = self._host(dist).reshape(-1), self._host(idx).reshape(-1)
        if (idx < 0).any():
            raise ValueError("a row of X has no prototype at a finite distance")
        if h is None:
            h2 = fsum((dist * dist).tolist()) / (n * X.shape[1])
            if not (np.isfinite(h2) and h2 > 0.0):
                raise ValueError(f"the bandwidth estimated from X is not a finite value > 0 (h^2 = {h2!r}): pass bandwidth")
            h = self._check_bandwidth(sqrt(h2))
        self.mixture_priors_ = np.bincount(idx, minlength=M).astype(np.float64) / n
        self.mixture_bandwidth_ = h
        return self

    def _mixture(self, X, what, values, bandwidth, priors):
        """-> (X, unit, lse, q, h) of the validated rows; no rows: empty host arrays without a launch"""
        X = self._mixture_query(X, what)
        a, c, h = self._mixture_params(bandwidth, priors)
        if X.shape[0] == 0 and not is_device_array(X):
            q = None if values is None else np.empty((0, values.shape[1]), dtype=np.float64)
            return X, np.empty(0, dtype=np.int64), np.empty(0, dtype=np.float64), q, h
        unit, lse, q = self._engine().mixture(self.weights_, a, c, values, X)
        return X, unit, lse, q, h

    def sample_mixture(self, X, bandwidth=None, priors=None):
        """``(log_density, map_unit)``, ``(n_samples,)`` float64 and int64: ``score_samples(X)`` and the unit with the
        largest posterior, ``argmax_j (log prior_j - ||x_i - w_j||^2 / (2 h^2))``, lowest index among equals -- with
        equal priors ``predict``'s unit for ``SomVQ``.  Both come from one pass.  A row for which no unit has mass has
        ``(NaN, -1)``.  Arguments, X and the refusals are ``score_samples``'s."""
        X, unit, lse, _, h = self._mixture(X, "sample_mixture / score_samples", None, bandwidth, priors)
        return lse - 0.5 * X.shape[1] * log(2.0 * pi * h * h), unit

    def score_samples(self, X, bandwidth=None, priors=None):
        """The log-density of every row under the map read as an isotropic Gaussian mixture, ``(n_samples,)`` float64:
        ``log p(x_i) = log sum_j prior_j exp(-||x_i - w_j||^2 / (2 h^2)) - (d / 2) log(2 pi h^2)`` -- a
        ``score_samples`` in scikit-learn's sense, and a novelty score: low where the map has no prototype nearby.

        ``bandwidth`` / ``priors`` ``None`` take ``mixture_bandwidth_`` / ``mixture_priors_`` (``fit_mixture``);
        without them a ``ValueError`` says so.  ``bandwidth`` is a finite float > 0; ``priors`` an array-like
        ``(len(weights_),)``, non-negative and summing to 1 within 1e-9, or ``"uniform"``.

        The squared distances are those of the best-matching-unit search's own arithmetic, ``r_ij = max((|x_i|^2 + (-2
        <x_i, w_j>)) + |w_j|^2, 0)``, the ones ``kneighbors`` selects on.  ``t_j = log prior_j - (c * r_ij)`` with ``c =
        1 / (2 h^2)`` (two roundings), the sum is ``T + log(sum_j exp(t_j - T))`` with T the largest ``t_j``, 64
        strided partials then six xor rounds, in float64 with the device library's ``exp`` and ``log``; the constant
        is added on the caller's side.  The order is fixed, so the result does not depend on chunks, slabs or where X
        lives.  The N x M matrix is never held.

        X is what ``sample_distortion`` takes: a dense array (a NumPy result; 16 bytes per row come down), a tensor on
        the estimator's GPU (a tensor on X's device; X never touches the host), scipy sparse rows (the dense call's
        result on ``X.toarray()``).  Refused with a ``ValueError``: ``metric="manhattan"`` / ``"cosine"`` (the model is
        Gaussian in the Euclidean distance), rows with NaN (also under ``missing_values``: impute them first), a
        feature-count mismatch.  Only this map's prototypes are used (not the child maps of vertical growth); the call
        is local to the process."""
        return self.sample_mixture(X, bandwidth, priors)[0]

    def calculate_log_likelihood(self, X, bandwidth=None, priors=None) -> float:
        """The mean of ``score_samples(X, bandwidth, priors)`` as a float.  The per-row values come to the host (8
        bytes per row) and NumPy sums them, so a host array and a tensor holding the same rows give the same float."""
        s = self.score_samples(X, bandwidth, priors)
        if s.shape[0] == 0:
            check_array(X, dtype=[np.float64, np.float32])   # (no rows: refused in check_array's words, as a mean is)
        return float(np.sum(self._host(s))) / s.shape[0]

    def posterior_mean(self, X, values, bandwidth=None, priors=None):
        """The posterior mean of a per-unit quantity: ``q_i = sum_j p(j | x_i) values[j]`` with ``p(j | x_i)`` the
        responsibilities of the mixture of ``score_samples`` -- class shares, a component plane, a label, read softly
        instead of at the best matching unit.  ``values`` is ``(len(weights_),)`` or ``(len(weights_), V)`` with ``V
        <= 16`` real numbers; the result is ``(n_samples,)`` or ``(n_samples, V)`` float64.  Every column is ``sum_j
        (s_j * values[j]) / sum_j s_j`` with ``s_j = exp(t_j - T)`` in the fixed order of ``score_samples``, one
        division per row and column.  A row for which no unit has mass has NaN.  From a dense array ``8 V`` bytes per
        row come down beside ``score_samples``'s 16.  Arguments, X and the refusals are ``score_samples``'s."""
        check_is_fitted(self)
        M = len(self.weights_)
        values = self._host(values)   # (a per-unit result that lives in HBM, unit_means of a tensor)
        try:
            Y = np.asarray(values, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError(f"values must be real numbers of shape ({M},) or ({M}, V), got {values!r}") from None
        flat = Y.ndim == 1
        if flat:
            Y = Y.reshape(-1, 1)
        if Y.ndim != 2 or Y.shape[0] != M or Y.shape[1] < 1:
            raise ValueError(f"values must have shape ({M},) or ({M}, V), one row per prototype, got {np.shape(values)}")
        if Y.shape[1] > MAX_MIXTURE_VALUES:
            raise ValueError(f"values has {Y.shape[1]} columns, above the {MAX_MIXTURE_VALUES} the kernel sums per row: "
                             "use several calls")
        q = self._mixture(X, "posterior_mean / project", np.ascontiguousarray(Y), bandwidth, priors)[3]
        return q[:, 0] if flat else q

    def project(self, X, bandwidth=None, priors=None):
        """The smooth projection of every row onto the lattice, ``(n_samples, 2)`` float64: the posterior mean of the
        units' lattice coordinates (the node tuples ``neurons_``, in the order of ``weights_``) -- GTM's "mean
        projection".  Rows between two units land between their nodes instead of collapsing onto one; every position
        lies inside the bounding box of the lattice.  ``posterior_mean(X, coordinates, bandwidth, priors)``."""
        check_is_fitted(self)
        return self.posterior_mean(X, np.asarray(list(self.neurons_), dtype=np.float64).reshape(len(self.weights_), -1),
                                   bandwidth, priors)

    # ------------------------------------------------------------------------------------------
    # a per-row quantity on the map
    # ------------------------------------------------------------------------------------------
    def _check_row_values(self, values, n, on_device, name="values"):
        """-> (float64 (n, V) values, flat): a host array, or with ``on_device`` a tensor left where it is"""
        say = (f"{name} must be real numbers of shape ({n},) or ({n}, V) with V <= {MAX_MIXTURE_VALUES}, one row per "
               f"row of X")
        if on_device and is_device_array(values):
            Z = values
            kind = dtype_name(Z)
            if not kind.startswith(("float", "bfloat", "int", "uint", "bool")):
                raise ValueError(f"{say}; got dtype {kind}")
            shape = tuple(int(v) for v in Z.shape)
        else:
            try:
                Z = np.asarray(self._host(values))
            except (TypeError, ValueError):
                raise ValueError(f"{say}; got {values!r}") from None
            if Z.dtype.kind not in "fiub":
                raise ValueError(f"{say}; got dtype {Z.dtype}")
            shape = Z.shape
        if len(shape) not in (1, 2):
            raise ValueError(f"{say}; got {len(shape)} dimensions (shape {shape})")
        if shape[0] != n:
            raise ValueError(f"{say}; got {shape[0]} rows for {n} rows of X")
        flat = len(shape) == 1
        V = 1 if flat else shape[1]
        if V < 1:
            raise ValueError(f"{say}; got no column")
        if V > MAX_MIXTURE_VALUES:
            raise ValueError(f"{name} has {V} columns, above the {MAX_MIXTURE_VALUES} the kernel sums per row: use "
                             "several calls")
        if isinstance(Z, np.ndarray):
            return np.ascontiguousarray(Z, dtype=np.float64).reshape(n, V), flat
        return (Z if dtype_name(Z) == "float64" else Z.double()).reshape(n, V), flat

    def _check_row_weights(self, sample_weight, n, on_device):
        """-> None or float64 (n,) weights, non-negative and finite: a host array, or with ``on_device`` a tensor"""
        if sample_weight is None:
            return None
        say = f"sample_weight must be {n} finite numbers >= 0, one per row of X"
        if on_device and is_device_array(sample_weight):
            w = sample_weight
            if len(w.shape) != 1 or int(w.shape[0]) != n:
                raise ValueError(f"{say}; got shape {tuple(int(v) for v in w.shape)}")
            w = w if dtype_name(w) == "float64" else w.double()
            ns = array_namespace(w)
            if not bool(ns.isfinite(w).all()) or not bool((w >= 0).all()):
                raise ValueError(f"{say}; got a negative or non-finite weight")
            return w
        try:
            w = np.asarray(self._host(sample_weight), dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError(f"{say}; got {sample_weight!r}") from None
        if w.shape != (n,):
            raise ValueError(f"{say}; got shape {w.shape}")
        if not np.isfinite(w).all() or not (w >= 0).all():
            raise ValueError(f"{say}; got a negative or non-finite weight")
        return np.ascontiguousarray(w)

    def unit_means(self, X, values, sample_weight=None, return_std=False, return_mass=False):
        """The component plane of an external variable: for every unit the weighted mean of ``values`` over the rows
        of X whose best matching unit it is -- ``(len(weights_),)`` for ``values`` of shape ``(n,)``, ``(len(weights_),
        V)`` for ``(n, V)`` with ``V <= 16``, float64, NaN for a unit without mass.  ``return_std`` adds the per-unit
        standard deviation ``sqrt(sum w (z - mean)^2 / sum w)`` in the same shape, ``return_mass`` the mass ``sum w``
        (the number of rows without weights), ``(len(weights_),)``: the result is then a tuple ``(mean[, std][,
        mass])``.  ``posterior_mean(Q, som.unit_means(X, z))`` reads the plane back at new rows.

        The units are ``predict``'s, so X is whatever ``predict`` takes: a host array, a tensor on the estimator's GPU
        (the results are tensors on its device; ``values`` and ``sample_weight`` may be host arrays or tensors), scipy
        sparse rows, rows with NaN under ``missing_values``, any ``metric``.  A row without a unit (-1) takes no part, a
        row of weight 0 neither (a NaN stored under weight 0 is never read); NaN and infinities in ``values`` are
        plain IEEE and reach their own (unit, column) only.

        The sums run on the GPU in a fixed order (csrc/unit_sums.hip): a unit's rows ascending, blocks of 128 added
        from +0.0, then the blocks ascending; the term of a row is ``w * z`` rounded once.  So a host array, a tensor and
        CSR rows of the same data give the same bits, and all-ones weights give the bits of no weights.  ``mean = sums /
        mass``, one division.  Refused with a ``ValueError``: ``values`` of the wrong length, rank or dtype or with more
        than 16 columns; a negative, non-finite or wrong-length ``sample_weight``."""
        check_is_fitted(self)
        X = self._check_query(X)
        n, on_device = int(X.shape[0]), is_device_array(X)
        Z, flat = self._check_row_values(values, n, on_device)
        w = self._check_row_weights(sample_weight, n, on_device)
        units = self._get_winning_neurons(X, n_bmu=1)[1]
        mass, mean, std, _ = self._engine().unit_statistics(units, Z, w, len(self.weights_), want_std=bool(return_std))
        out = [mean[:, 0] if flat else mean]
        if return_std:
            out.append(std[:, 0] if flat else std)
        if return_mass:
            out.append(mass)
        return out[0] if len(out) == 1 else tuple(out)

    def _lattice_edges(self) -> np.ndarray:
        """The undirected edges of the fitted lattice as an (E, 2) int32 array of indices into ``weights_`` /
        ``neurons_`` (the graph as it is after the dead units were removed; it survives a pickle)."""
        index = {n: i for i, n in enumerate(self.neurons_)}
        edges = [(index[a], index[b]) for a, b in self.som_.edges]
        return np.asarray(edges, dtype=np.int32).reshape(-1, 2)

    def prototype_geodesics(self) -> np.ndarray:
        """The weighted geodesic distances over the lattice: an ``(M, M)`` float64 array in the order of ``weights_``
        / ``neurons_``.  A lattice edge is as long as its two prototypes are apart in the input space, ``len(a, b) =
        sqrt(sum_k (w_ak - w_bk)^2)`` summed k ascending with every operation rounded on its own, and ``G[s, t]`` is
        the length of the shortest path from s to t, its lengths added from s on; ``G[s, s] = 0`` and ``+inf``
        between components.  The minimum is unique whatever order the edges are relaxed in (rounded addition of a
        non-negative length is monotone).  ``G[s, t]`` and ``G[t, s]`` add the same lengths from different ends and
        differ in their last bits for most pairs; the matrix is not symmetrised.  This is what geodesic clustering of
        the prototypes and U-matrix-style views are built from.  Only this map's prototypes are used; the call is
        local to the process."""
        check_is_fitted(self)
        return self._engine().geodesics(self.weights_, self._lattice_edges())

    def sample_combined_error(self, X):
        """The combined error of Kaski and Lagus (1996) row by row: ``(e, units)``, ``(n_samples,)`` float64 and
        ``(n_samples, 2)`` int64, with ``units[i] = (b1, b2)`` the best and second-best matching unit of row ``i``
        (``units[:, 0]`` is ``predict``'s unit for ``SomVQ``) and ``e_i = ||x_i - w_b1|| + G[b1, b2]``, G the
        ``prototype_geodesics()`` of the map: the quantization error of the row plus the way along the map from its
        unit to the runner-up.  Continuous and free of a bandwidth, so the usual choice for comparing maps of
        different size; ``+inf`` where the two units lie in different components of the lattice.

        The two distances are those of the best-matching-unit search's own arithmetic without float32 rounding, ties
        go to the lower index, and the sum is one rounded addition, so the result does not depend on chunks or where X
        lives.  G is computed on the GPU once per call.

        X is what ``kneighbors`` takes under the Euclidean metric: a dense array (NumPy results), a tensor on the
        estimator's GPU (tensors on X's device), scipy sparse rows (the dense call's result on ``X.toarray()``).
        Refused with a ``ValueError``: ``metric="manhattan"`` / ``"cosine"`` (the measure is defined on Euclidean
        distances), rows with NaN (also under ``missing_values``: impute them first), a feature-count mismatch, a
        map of fewer than two prototypes.  Only this map's prototypes are used (not the child maps of vertical
        growth); the call is local to the process."""
        check_is_fitted(self)
        kind = self._search_metric()
        if kind:
            self._refuse_metric(kind, "sample_combined_error / calculate_combined_error",
                                "the measure is defined on Euclidean distances")
        if len(self.weights_) < 2:
            raise ValueError(f"the combined error needs a map of at least two prototypes, this one has "
                             f"{len(self.weights_)}")
        if not is_device_array(X) and not is_sparse(X) and np.ndim(X) == 2 and np.shape(X)[0] == 0:
            X = check_array(X, dtype=[np.float64, np.float32], ensure_min_samples=0)   # (no rows: no launch)
        else:
            X = self._check_query(X)
        if X.shape[1] != self.n_features_in_:
            raise ValueError(f"X has {X.shape[1]} features, but {type(self).__name__} is expecting "
                             f"{self.n_features_in_} features as input")
        if isinstance(X, np.ndarray) and np.isnan(X).any():   # (passed _check_query: missing_values is set)
            raise ValueError(f"X holds NaN: the combined error is not defined on rows with missing entries "
                             f"(missing_values={self.missing_values!r}); impute them first (impute(X))")
        if X.shape[0] == 0:
            return np.empty(0, dtype=np.float64), np.empty((0, 2), dtype=np.int64)
        return self._engine().combined_error(self.weights_, self._lattice_edges(), X)

    def calculate_combined_error(self, X) -> float:
        """The combined error of X: the mean of ``sample_combined_error(X)[0]``.  The per-row values come to the host
        (8 bytes per row) and NumPy sums them, so a host array, a tensor and sparse rows holding the same data give
        the same float.  ``+inf`` when some row's two units lie in different components of the lattice: that is the
        measure's value there."""
        e, _ = self.sample_combined_error(X)
        if e.shape[0] == 0:
            check_array(X, dtype=[np.float64, np.float32])   # (no rows: refused in check_array's words, as a mean is)
        return float(np.sum(self._host(e))) / e.shape[0]

    def _calculate_topographic_error(self, X) -> float:
        """Fraction of samples whose two best matching units are not lattice neighbours."""
        if self._is_resident(X):
            return self._engine().topographic_error_count(self.weights_, self.neurons_) / self._n_effective()
        _, bmu = self._get_winning_neurons(X, n_bmu=2)
        pos = np.asarray(list(self.neurons_), dtype=np.float64)
        apart = np.linalg.norm(pos[bmu[:, 0]] - pos[bmu[:, 1]], axis=1) > 1.5
        return int(np.count_nonzero(apart)) / X.shape[0]

    def _get_u_matrix(self) -> np.ndarray:
        """Mean input-space distance from every prototype to the list of all neighbour
        prototypes (the reference averages over the WHOLE concatenated list, :320-337)."""
        lat = self._lattice
        nbr_rows = [lat.index_of(nb) for nbrs in lat.graph.adj.values() for nb in nbrs]
        return scipy.spatial.distance.cdist(lat.W, lat.W[nbr_rows]).mean(axis=1)

    def _calculate_node_statistics(self, X):
        average_distances = self._get_u_matrix()
        sigma = average_distances.mean()
        m = len(self._lattice)  # neurons inserted in the very last epoch count as dead
        if self._is_resident(X):
            hits, sums = self._engine().node_statistics(self.weights_, sigma)
        else:
            distances, winners = self._get_winning_neurons(X, n_bmu=1)
            hits = np.bincount(winners, minlength=len(self.weights_)).astype(np.float64)
            dens = np.exp(-(distances ** 2) / (2 * sigma ** 2)) / (sigma * sqrt(2 * pi))
            sums = np.bincount(winners, weights=dens, minlength=len(self.weights_))
        hit_counts, dens_sums = np.zeros(m), np.zeros(m)
        hit_counts[: len(hits)], dens_sums[: len(sums)] = hits, sums
        densities = np.divide(dens_sums, hit_counts, out=np.zeros(m), where=hit_counts > 0)
        return average_distances, densities, hit_counts

    def _write_node_statistics(self, X) -> None:
        avg, dens, hits = self._calculate_node_statistics(X)
        self._node_stats = {"density": dens, "hit_count": hits, "average_distance": avg}
        self._lattice.write_attributes(self._node_stats)

    def _delete_dead_neurons_from_graph(self, X) -> None:
        lat = self._lattice
        hits = self._node_stats["hit_count"]
        keep = hits != 0
        dead = [n for n, h in zip(lat.nodes, hits) if h == 0]
        lat.remove(dead)
        self._node_stats = {k: v[keep] for k, v in self._node_stats.items()}
        lat.write_attributes(self._node_stats)
        self._sync_views(refresh_weights=True)  # weights_ now holds the last update

    def _extract_values_from_graph(self, attribute: str) -> np.ndarray:
        return np.array([data[attribute] for _, data in self.som_.nodes.data()])

    # ------------------------------------------------------------------------------------------
    # parts of the surface outside the accelerated path (kept for drop-in completeness)
    # ------------------------------------------------------------------------------------------
    def transform(self, X, y=None) -> np.ndarray:
        """Non-negative LARS-lasso code of X over the prototypes (BaseSom.py:241-268): scikit-learn's
        SparseCoder on normalize(X) with dictionary normalize(weights_), computed by the backend
        (on the MI355X: csrc/sparse_code.hip; n_jobs only matters to the host default)."""
        check_is_fitted(self)
        X = self._complete_query(self._check_query(X))
        return self._sparse_code(X)

    _SPARSE_CODE_ROWS = 4096   # rows of sparse X densified at a time for the sparse coder

    def _sparse_code(self, X, P=None):
        """The backend's sparse code (class probabilities with P) of the rows of X.  Sparse X: row chunks are
        densified on the host into the same call -- rows are coded independently, so the result is the dense
        call's."""
        engine = self._engine()
        if not is_sparse(X):
            return engine.sparse_code(self.weights_, X, P=P, n_jobs=self.n_jobs)
        step = self._SPARSE_CODE_ROWS
        parts = [engine.sparse_code(self.weights_, X[lo:lo + step].toarray(), P=P, n_jobs=self.n_jobs)
                 for lo in range(0, X.shape[0], step)]
        return np.concatenate(parts, axis=0)

    def topographic_function(self, X) -> tuple[np.ndarray, np.ndarray]:
        """(phi(k) / M for k = 0 .. max_dist - 1, phi(-k) / M for the same k), max_dist the largest
        Chebyshev distance between lattice positions (BaseSom.py:955-998).  The graph is the induced
        Delaunay triangulation of X (an edge between the two BMUs of every sample); the backend returns
        the two histograms phi is made of (on the MI355X: csrc/topofn.hip).  Unlike the reference, no
        dense M x M matrix is kept on the estimator (``want_distances=True`` on the backend gives D).
        Dense X only: sparse X raises ``TypeError``."""
        check_is_fitted(self)
        if self._search_metric():
            self._refuse_metric(self._search_metric(), "topographic_function",
                                "its induced Delaunay graph is built on the Euclidean search")
        X = self._check_device_array(X, fit=False) if is_device_array(X) else check_array(X, dtype=[np.float64, np.float32])
        if X.shape[1] != self.n_features_in_:
            raise ValueError(f"X has {X.shape[1]} features, but {type(self).__name__} is expecting "
                             f"{self.n_features_in_} features as input")
        M = len(self.neurons_)
        if M < 2:
            raise ValueError(f"Expected n_neighbors <= n_samples_fit, but n_neighbors = 2, n_samples_fit = {M}")
        hist_pos, hist_neg, _ = self._engine().topographic_function(self.weights_, X, self.neurons_)
        self._topofn_hist_pos = np.asarray(hist_pos, dtype=np.int64)
        self._topofn_hist_neg = np.asarray(hist_neg, dtype=np.int64)
        max_dist = len(self._topofn_hist_pos) - 1
        k_pos = np.array([self.phi(k) for k in range(max_dist)], dtype=np.int64)
        k_neg = np.array([self.phi(-k) for k in range(max_dist)], dtype=np.int64)
        return k_pos / M, k_neg / M

    def phi(self, k: int) -> int:
        """Ordered pairs of neurons (i, j) with, for k > 0, a Delaunay edge between them and a
        Chebyshev lattice distance > k; for k < 0, lattice neighbours more than -k hops apart in the
        Delaunay graph (or with no path); phi(0) = phi(-1) + phi(1) (BaseSom.py:983-995).  Answers
        from the histograms of the last ``topographic_function`` call."""
        hist_pos, hist_neg = self._topofn_hist_pos, self._topofn_hist_neg
        k = int(k)
        if k > 0:
            return int(hist_pos[k + 1:].sum())
        if k < 0:
            M = len(hist_neg) - 1  # hist_neg[M]: no path, more than any number of hops
            return int(hist_neg[min(-k + 1, M):].sum())
        return self.phi(-1) + self.phi(1)

    def _grow_vertical(self, X, y=None) -> None:
        """Fit a child map on the Voronoi set of every neuron whose error exceeds 1.5x the
        growing threshold (BaseSom.py:157-179).  The reference's own loop cannot run: it compares
        the (node, error) tuple with a float (TypeError) and would index the graph by position;
        this is the evident intent, pinned by tests/golden/vertical_*.npz (made with exactly
        those two slips corrected, tools/make_golden.py).  On the MI355X the Voronoi sets are
        gathered in HBM (dbgsom_ctx_partition / dbgsom_ctx_subset_create): no X[mask] on the
        host, no second upload."""
        self.vertical_growing_threshold_ = 1.5 * self.growing_threshold_
        engine = self._engine()
        errors = self._lattice.error
        # (sparse X: the host-subset branch -- X[winners == j] is CSR row selection)
        on_device = self._is_resident(X) and hasattr(engine, "subset") and dist_info()[1] == 1 and not is_sparse(X)
        sw = self._sw
        if isinstance(X, DeviceSamples) and not on_device:
            raise ValueError("vertical_growth=True on device rows needs a backend that gathers Voronoi subsets on the "
                             "device and one process; " + self._HOST_ARRAY)
        if on_device:
            counts, winners = engine.partition(self.weights_, want_winners=y is not None or sw is not None)
        else:
            _, winners = self._get_winning_neurons(X, n_bmu=1)
            counts = np.bincount(winners, minlength=len(self.neurons_))
        if sw is not None:   # a Voronoi set is as large as its rows' summed weight
            counts = np.bincount(winners, weights=sw, minlength=len(self.neurons_))
        for j, node in enumerate(self.neurons_):
            if not errors[j] > self.vertical_growing_threshold_:
                continue
            if counts[j] > self.min_samples_vertical_growth:
                child = clone(self)
                y_sub = None if y is None else y[winners == j]
                w_sub = {} if sw is None else {"sample_weight": sw[winners == j]}
                if on_device:
                    sub = engine.subset(j)
                    child._backend_obj = sub
                    child.fit(DeviceSamples(sub), y_sub, **w_sub)
                else:
                    child.fit(X[winners == j], y_sub, **w_sub)
                self.som_.nodes[node]["som"] = child

    def plot(self, color=None, palette="magma_r", pointsize=None) -> None:
        """Scatter of the lattice coloured by a node attribute (needs seaborn >= 0.12)."""
        import pandas as pd
        import seaborn.objects as so

        data = pd.DataFrame(dict(self.som_.nodes)).T.reset_index(drop=True)
        for col in ("epoch_created", "error", "density", "hit_count", "average_distance"):
            if col in data:
                data[col] = pd.to_numeric(data[col])
        xy = pd.DataFrame(np.array(self.neurons_), columns=["x", "y"])
        so.Plot(pd.concat([xy, data], axis=1), x="x", y="y", color=color,
                pointsize=pointsize).add(so.Dot()).scale(color=palette).label(x="", y="").show()
