"""Supervised estimator for a continuous target: a growing SOM whose units carry the mean of y.

``fit(X, y)`` trains the map on X, then puts y on the units: ``unit_targets_[j]`` is the (weighted) mean of y over the
rows whose best matching unit is j, ``unit_target_std_`` their spread and ``unit_mass_`` their number (summed weight),
from one pass of per-unit sums on the GPU (csrc/unit_sums.hip, ``backend.unit_statistics``).  ``predict`` reads the
units back at the best matching unit (``prediction="bmu"``), between the nearest units (``"knn"``) or through the
map's mixture (``"soft"``).

``growth_criterion="target_error"`` lets the target drive the directed growth: the error a unit accumulates per epoch
is ``sum over its rows of w_i ||y_i - mean_j||_2`` instead of the summed distance in X, so the map grows where the
target is badly explained, not where X is spread out.  The default stays ``"quantization_error"``.
"""
from __future__ import annotations

import numpy as np
from sklearn.base import RegressorMixin
from sklearn.utils.validation import check_is_fitted

from ._native import MAX_MIXTURE_VALUES
from .backend import array_namespace, dist_info, is_device_array
from .base import BaseSom


class SomRegressor(BaseSom, RegressorMixin):
    """Directed batch growing SOM regressor (see ``BaseSom`` for the shared parameters).

    prediction   "bmu" (default): ``unit_targets_`` of the best matching unit; "knn": the mean over the
                 ``min(n_neighbors, len(weights_))`` nearest units weighted by 1 / distance; "soft":
                 ``posterior_mean(X, unit_targets_)`` (needs ``fit_mixture``)
    n_neighbors  the units "knn" averages over

    Fitted attributes beside BaseSom's: ``n_outputs_``, ``unit_targets_``, ``unit_target_std_`` (both
    ``(len(weights_),)`` for 1-D y, ``(len(weights_), T)`` otherwise; NaN for a unit that ends without a row) and
    ``unit_mass_`` ``(len(weights_),)``."""

    _GROWS_ON_TARGETS = True
    _PREDICTIONS = ("bmu", "knn", "soft")
    _CRITERIA = ("quantization_error", "target_error")

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
        prediction: str = "bmu",
        n_neighbors: int = 5,
    ) -> None:
        super().__init__(
            n_iter=n_iter, convergence_iter=convergence_iter, spreading_factor=spreading_factor, sigma_start=sigma_start,
            sigma_end=sigma_end, vertical_growth=vertical_growth, decay_function=decay_function,
            learning_rate=learning_rate, verbose=verbose, coarse_training_frac=coarse_training_frac,
            random_state=random_state, convergence_treshold=convergence_treshold, max_neurons=max_neurons, metric=metric,
            threshold_method=threshold_method, growth_criterion=growth_criterion,
            min_samples_vertical_growth=min_samples_vertical_growth, n_jobs=n_jobs, backend=backend,
            centres_layout=centres_layout, device=device, sharded_input=sharded_input, init=init,
            initial_shape=initial_shape, missing_values=missing_values)
        self.prediction = prediction
        self.n_neighbors = n_neighbors

    # -- fit ---------------------------------------------------------------------------------------------
    def _check_prediction(self) -> None:
        if self.prediction not in self._PREDICTIONS:
            raise ValueError(f"SomRegressor: prediction must be one of {self._PREDICTIONS}, got {self.prediction!r}")
        k = self.n_neighbors
        if isinstance(k, (bool, np.bool_)) or not isinstance(k, (int, np.integer)) or k < 1:
            raise ValueError(f"SomRegressor: n_neighbors must be an integer >= 1, got {k!r}")

    def _check_input_data(self, X, y):
        self._check_prediction()
        if self.vertical_growth:
            raise ValueError("SomRegressor does not take vertical_growth=True: the units of one map carry the targets; "
                             "pass vertical_growth=False")
        if self.sharded_input or dist_info()[1] > 1:
            raise ValueError("SomRegressor takes one process: no sharded_input, no process group of more than one rank")
        if self.growth_criterion not in self._CRITERIA:
            raise ValueError(f"SomRegressor: growth_criterion must be one of {self._CRITERIA} -- 'entropy' is a criterion "
                             f"for class labels --, got {self.growth_criterion!r}")
        if y is None:
            raise ValueError("SomRegressor requires y to be passed, but the target y is None")
        X, _ = self._check_fit_array(X)
        X = self._check_sparse_input(X)
        n = int(X.shape[0])
        try:
            Y = np.asarray(self._host(y), dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError(f"SomRegressor: y must be real numbers of shape ({n},) or ({n}, T)") from None
        if Y.ndim not in (1, 2) or Y.shape[0] != n or (Y.ndim == 2 and Y.shape[1] < 1):
            raise ValueError(f"SomRegressor: y must have shape ({n},) or ({n}, T), one row per row of X, got {Y.shape}")
        if Y.ndim == 2 and Y.shape[1] > MAX_MIXTURE_VALUES:
            raise ValueError(f"SomRegressor: y has {Y.shape[1]} columns, above the {MAX_MIXTURE_VALUES} outputs the "
                             "per-unit sums take: fit one regressor per group of columns")
        if not np.isfinite(Y).all():
            raise ValueError("SomRegressor: y holds NaN or an infinity")
        return X, np.ascontiguousarray(Y)

    def _encode_targets(self, y):
        """y stays float64: (n, T) for the fit, ``n_outputs_`` = T; no ``classes_``."""
        self._y_flat = y.ndim == 1
        Y = np.ascontiguousarray(y.reshape(len(y), -1))
        self.n_outputs_ = int(Y.shape[1])
        self._fit_targets = Y
        return Y

    def fit(self, X, y, sample_weight=None):
        """Train the map on X (``BaseSom.fit``: X and ``sample_weight`` are what ``SomVQ.fit`` takes, sparse rows and
        tensors included) and put y on its units.  y: ``(n,)`` or ``(n, T)`` with ``T <= 16``, finite, a host array or a
        tensor (it goes to the host).  Refused with a ``ValueError``: ``vertical_growth=True``, ``sharded_input`` or
        more than one rank, ``growth_criterion="entropy"``, more than 16 outputs."""
        try:
            return super().fit(X, y, sample_weight=sample_weight)
        finally:
            self.__dict__.pop("_fit_targets", None)

    def _label_prototypes(self, X, y) -> None:
        """Mean, spread and mass of y per unit from one call of per-unit sums on the winners of the resident rows."""
        winners = self._resident_winners(X)
        mass, mean, std, _ = self._engine().unit_statistics(winners, y, self._sw, len(self.neurons_), want_std=True)
        mass, mean, std = (np.asarray(self._host(a)) for a in (mass, mean, std))
        self.unit_mass_ = mass
        self.unit_targets_ = mean[:, 0] if self._y_flat else mean
        self.unit_target_std_ = std[:, 0] if self._y_flat else std
        self._lattice.write_attributes({"target": list(mean), "target_std": list(std)})

    # -- predict -----------------------------------------------------------------------------------------
    def _unit_table(self, table, like):
        """A per-unit attribute as an (M, T) array in X's namespace"""
        table = np.ascontiguousarray(np.asarray(table, dtype=np.float64).reshape(len(self.weights_), -1))
        return self._like(table, like) if is_device_array(like) else table

    @staticmethod
    def _take(table, idx):
        """table[idx] with NaN rows where idx is negative (the search reported no unit)"""
        ns = np if isinstance(table, np.ndarray) else array_namespace(table)
        missing = idx < 0
        out = table[ns.where(missing, 0, idx)]
        return ns.where(missing[:, None], float("nan"), out)

    def predict(self, X, return_std=False):
        """The target of every row: ``(n,)`` for a 1-D y, ``(n, T)`` otherwise; from a tensor a tensor on its device.

        "bmu": ``unit_targets_[bmu]``, NaN where the search reports no unit; with ``return_std`` the result is
        ``(prediction, unit_target_std_[bmu])``.  "knn": ``kneighbors(X, min(n_neighbors, len(weights_)))`` with
        weights ``1 / dist``, accumulated neighbour by neighbour in X's own array namespace (``num = num + w_t *
        Y[idx_t]``, ``den = den + w_t``, ``num / den``: elementwise operations only, so a host array and a tensor
        agree bit for bit); a row whose first distance is 0 takes that unit's value, and with one neighbour the mean of
        one value is that value: "knn" equals "bmu".  "soft": ``posterior_mean(X, unit_targets_)``; without
        ``fit_mixture`` that call's ``ValueError``.  ``return_std`` is "bmu"'s alone."""
        check_is_fitted(self)
        self._check_prediction()
        if return_std and self.prediction != "bmu":
            raise ValueError(f"SomRegressor: return_std needs prediction='bmu' (the spread of one unit), got "
                             f"prediction={self.prediction!r}")
        flat = self._y_flat
        if self.prediction == "soft":
            return self.posterior_mean(X, self.unit_targets_)
        if self.prediction == "knn":
            k = min(int(self.n_neighbors), len(self.weights_))
            dist, idx = self.kneighbors(X, k)
            Y = self._unit_table(self.unit_targets_, dist)
            if k == 1:
                out = self._take(Y, idx[:, 0])
                return out[:, 0] if flat else out
            ns = np if isinstance(dist, np.ndarray) else array_namespace(dist)
            num = den = None
            with np.errstate(all="ignore"):
                for t in range(k):
                    wt = 1.0 / dist[:, t]
                    miss = idx[:, t] < 0                      # (an unfilled slot: (inf, -1), weight 0)
                    term = ns.where(miss[:, None], 0.0, wt[:, None] * Y[ns.where(miss, 0, idx[:, t])])
                    num = term if num is None else num + term
                    den = wt if den is None else den + wt
                out = num / den[:, None]
            out = ns.where((dist[:, 0] == 0)[:, None], self._take(Y, idx[:, 0]), out)
            return out[:, 0] if flat else out
        X = self._check_query(X)
        idx = self._get_winning_neurons(X, n_bmu=1)[1]
        out = self._take(self._unit_table(self.unit_targets_, idx), idx)
        out = out[:, 0] if flat else out
        if not return_std:
            return out
        std = self._take(self._unit_table(self.unit_target_std_, idx), idx)
        return out, (std[:, 0] if flat else std)

    def score(self, X, y, sample_weight=None):
        """R^2 of ``predict(X)`` against y (``sklearn.metrics.r2_score``); predictions made on a device come to the
        host here."""
        from sklearn.metrics import r2_score

        pred = np.asarray(self._host(self.predict(X)))
        return float(r2_score(np.asarray(self._host(y)), pred,
                              sample_weight=None if sample_weight is None else np.asarray(self._host(sample_weight))))
