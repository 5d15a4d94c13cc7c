"""Models written in Python: the reference's extension point ("a *Def mixin and a dynamics function", i2c/env_def.py:34-82,
233-298, i2c/env_autograd.py:5-19) on the MI355X build. A TracedModel states its functions ONCE, as functions of scalars:

    class MyModel(TracedModel):
        dim_x, dim_u, dim_z, dim_z_term = 2, 1, 4, 2
        def __init__(self):
            super().__init__(); self.x0 = ...; self.sig_x0 = ...; self.sig_eta = ...; self.xag = ...; self.xu_lim = ...
        def device_params(self): return [mu, dt, u_max]
        def dynamics_fn(self, xu, p, m): ...           # xu: d scalars, p: NP scalars, m: the math namespace -> dim_x expressions
        def observe_fn(self, xu, p, m): ...            # -> dim_z expressions
        def observe_terminal_fn(self, x, p, m): ...    # -> dim_z_term expressions ([] when 0)
        # optional: measure_fn(self, x, p, m); default: observe_terminal_fn, as KnownModel.measure

`m` offers what a device functor may use (csrc/i2c_linearize.hpp): sin, cos, exp, clip(x, lo, hi), rcp, pi, next to + - * / and
integer powers. The same functions serve three callers: NumPy columns with m = NumpyMath (the host-side protocol dynamics /
observe / observe_terminal / measure, which the oracle takes too), sympy symbols (functor_codegen.py: the device functor, its
structure hints and family knobs, optionally its analytic Jacobian), and nothing else -- there is no second statement of the
model. resolve_model_id() emits the header under lib/generated/, builds the model library on first use and registers it; the
model is a plugin (id >= 64), as one brought by a hand-written header is.

A class that sets `operations = "extended"` widens `m` by sqrt, tanh, log, abs, minimum, maximum and where_gt(a, b, x, y) (x where
a > b, else y), may use Python's abs() and half-integer powers (x ** 0.5, x ** -1.5), and may take the sine of anything: of a
parameter, a product, an action. Such a functor calls r_sqrt / r_tanh / r_sincos itself, which pins their polynomial constants in
registers in every kernel it is instantiated in -- hence the statement. The default, "basic", is guaranteed to call no sine and
no square root. How each operation differentiates (abs' = sign and 0 at 0; min / max: the first argument at a tie; where_gt: the
selected branch; sqrt: a zero tangent stays zero at 0) is stated in csrc/i2c_linearize.hpp and INTEGRATION.md section 3. Still
outside: atan2 and the inverse functions, other fractional powers, a Python branch on a traced value. Write a model continuous
across its kinks: a sigma point within rounding of one must not move a result by more than rounding.
"""
import importlib.util
import os
import sys
import threading

import numpy as np

from .known_models import KnownModel


class NumpyMath:
    """The operation set on NumPy arrays (or floats)."""
    pi = np.pi
    sin, cos, exp, clip = staticmethod(np.sin), staticmethod(np.cos), staticmethod(np.exp), staticmethod(np.clip)
    # operations = "extended" (sqrt, tanh and log are complex-analytic: the host side still takes complex points through them)
    sqrt, tanh, log, abs = staticmethod(np.sqrt), staticmethod(np.tanh), staticmethod(np.log), staticmethod(np.abs)
    minimum, maximum = staticmethod(np.minimum), staticmethod(np.maximum)

    @staticmethod
    def rcp(x):
        return 1.0 / x

    @staticmethod
    def where_gt(a, b, x, y):
        return np.where(np.asarray(a) > np.asarray(b), x, y)


_LOAD_LOCK = threading.Lock()


def _codegen():
    """functor_codegen.py (next to the package's build.py), loaded once per process."""
    name = "i2c_amd_functor_codegen"
    with _LOAD_LOCK:
        return sys.modules[name] if name in sys.modules else _load_codegen(name)


def _load_codegen(name):
    pkg_dir = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location(name, os.path.join(pkg_dir, "functor_codegen.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    sys.modules[name] = mod
    return mod


class TracedModel(KnownModel):
    name = "Traced"
    traced = True      # (the device functor is generated on first use: there is no hip_header to name beforehand)
    knobs = None      # overrides of the derived family knobs, e.g. {"QUAD": False, "QUAD_FORWARD_MAX_B": 4096}
    jacobian = True    # emit jacobian<FN, R>() for Linearize() (False: dual-number passes, as for a hand-written functor)
    xag_term = None    # terminal target where it is not xag
    struct_name = None  # base name of the device struct and its files (default: the class name)
    operations = "basic"  # "extended": sqrt, tanh, log, abs, minimum, maximum, where_gt, half-integer powers, sines of anything

    def __init__(self, model=None, model_def=None, knobs=None, jacobian=None):
        super().__init__(model, model_def)
        if knobs is not None:
            self.knobs = dict(knobs)
        if jacobian is not None:
            self.jacobian = bool(jacobian)

    # ---- the model, stated once ---------------------------------------------------------------------------------------------
    def dynamics_fn(self, xu, p, m):
        raise NotImplementedError(f"{type(self).__name__}.dynamics_fn")

    def observe_fn(self, xu, p, m):
        raise NotImplementedError(f"{type(self).__name__}.observe_fn")

    def observe_terminal_fn(self, x, p, m):
        raise NotImplementedError(f"{type(self).__name__}.observe_terminal_fn")

    def measure_fn(self, x, p, m):
        return self.observe_terminal_fn(x, p, m)

    def process_noise_fn(self, xu, p, m):
        """OPTIONAL: the state-action-dependent part Q(xu) of the one-step covariance (a point's covariance is sig_eta + Q(xu)): the
        sym(nx) packed-lower (row-major) expressions, or the full nx x nx matrix as rows. Same operation set as dynamics_fn. A class
        that does not override it has constant noise, and its device functor is the one it always was."""
        return None

    @property
    def has_process_noise(self):
        return type(self).process_noise_fn is not TracedModel.process_noise_fn

    @property
    def dim_y(self):
        """Number of outputs of measure_fn (counted once: it is a property of the class's functions)."""
        if getattr(self, "_dim_y", None) is None:
            self._dim_y = len(list(self.measure_fn([0.0] * self.dim_x, [1.0] * len(self.device_params()), NumpyMath) or []))
        return self._dim_y

    @property
    def zg_term(self):
        if self.xag_term is not None:
            return self.xag_term
        if self.xag is not None and len(self.xag) == self.dim_z_term:
            return self.xag
        return self.zg

    # ---- host side: the same functions on NumPy columns (any leading axes, as the oracle's protocol) -------------------------------
    def _numpy(self, fn, v, n_in, n_out):
        v = np.asarray(v)
        if not np.iscomplexobj(v):  # (complex points pass through: complex-step differentiation of the host side)
            v = v.astype(float)
        assert v.shape[-1] == n_in, f"{type(self).__name__}: expected {n_in} columns, got {v.shape}"
        out = list(fn([v[..., i] for i in range(n_in)], [float(q) for q in self.device_params()], NumpyMath))
        assert len(out) == n_out, f"{type(self).__name__}.{fn.__name__} returned {len(out)} expressions, not {n_out}"
        if not out:
            return None
        return np.stack([np.broadcast_to(np.asarray(o, dtype=v.dtype), v.shape[:-1]) for o in out], axis=-1)

    def dynamics(self, xu):
        return self._numpy(self.dynamics_fn, xu, self.dim_xu, self.dim_x)

    def observe(self, xu):
        return self._numpy(self.observe_fn, xu, self.dim_xu, self.dim_z)

    def observe_terminal(self, x):
        return self._numpy(self.observe_terminal_fn, x, self.dim_x, self.dim_z_term)

    def measure(self, x):
        return self._numpy(self.measure_fn, x, self.dim_x, self.dim_y)

    def process_noise(self, xu):
        if not self.has_process_noise:
            return None
        nx = self.dim_x
        packed = self._numpy(lambda v, p, m: _codegen().pack_lower(self.process_noise_fn(v, p, m), nx), xu, self.dim_xu, nx * (nx + 1) // 2)
        r, c = np.tril_indices(nx)
        q = np.zeros(packed.shape[:-1] + (nx, nx))
        q[..., r, c] = packed
        q[..., c, r] = packed
        return q

    # ---- device side ----------------------------------------------------------------------------------------------------------
    def trace(self):
        """The traced expressions (functor_codegen.Spec); raises ValueError for anything a functor cannot hold."""
        cg = _codegen()
        who = type(self).__name__
        nzt = int(self.dim_z_term or 0)
        dims = {"NX": int(self.dim_x), "NU": int(self.dim_u), "NZ": int(self.dim_z), "NZT": nzt, "NY": 0}
        n_params = len(self.device_params())
        cg.check_limits(dims, n_params, who)
        dims["NY"] = self.dim_y
        fns = {"dynamics": self.dynamics_fn, "observe": self.observe_fn, "observe_terminal": self.observe_terminal_fn,
               "measure": self.measure_fn}
        if self.has_process_noise:
            fns["process_noise"] = self.process_noise_fn
        if self.operations == "basic":
            return cg, cg.trace(dims, fns, n_params, who)
        return cg, cg.trace(dims, fns, n_params, who, operations=self.operations)

    def header_text(self):
        """-> (codegen module, struct name, text, file stem); the struct is `<class or struct_name>_<hash of the text>`."""
        cg, spec = self.trace()
        # (the text -- and with it the library's name -- depends on the class's name and functions, not on how its module was imported)
        origin = f"the Python class {type(self).__name__}" + (f' (operations = "{self.operations}")' if spec.extended else "")
        text, struct, stem = cg.emit_unique(spec, self.struct_name or type(self).__name__, jacobian=self.jacobian, knobs=self.knobs,
                                            origin=origin)
        return cg, struct, text, stem

    def emit(self, out_dir=None):
        """Write the header (only when its text changed) and point hip_header / hip_struct / hip_name at it. -> the header's path"""
        cg, struct, text, stem = self.header_text()
        self.hip_header, self.hip_struct, self.hip_name = cg.write_header(text, stem, out_dir), struct, stem
        return self.hip_header

    def resolve_model_id(self, lib):
        """Traced and emitted on EVERY call (0.05 - 0.5 s): whatever the functions read -- an attribute, `knobs`, `jacobian` -- may have
        changed since the last one, and the device must follow the NumPy side. An unchanged model gives the same text, so the same
        file (not rewritten), the same library and, through the id cache of KnownModel.resolve_model_id, the same id."""
        self.emit()
        return super().resolve_model_id(lib)
