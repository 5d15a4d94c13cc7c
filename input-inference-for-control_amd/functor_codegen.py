"""A model written in Python -> the device functor header the kernels instantiate.

    spec = trace(dims, {"dynamics": fn, "observe": fn, "observe_terminal": fn, "measure": fn}, n_params)
    text, struct, stem = emit_unique(spec, "MyModel", jacobian=True, knobs={...})   # struct MyModel_<hash of the text>
    path = write_header(text, stem)            # lib/generated/my_model_<hash>.hpp, written only when it differs

The model functions are called ONCE with sympy symbols (`fn(xu, p, m)`: sequences of scalars and the math namespace `m` of
sym_math()): what comes back is the expression graph of every output. From it this module derives what a hand-written functor
states by hand (csrc/i2c_models.hpp):
  * the angle coordinates (NA, ang): inputs whose sine / cosine occurs; integer combinations of inputs plus a constant are expanded
    by angle addition, any other argument is refused; the body reads sn[a] / cs[a] and never calls a sine;
  * the structure hints (obs_lin / obs_dep ...): pass-through outputs and the largest input a general output depends on;
  * the family knobs: GROUP = the narrowest group that holds a row per lane, QUAD = whether the quad kernels accept the model (the
    conditions and static_asserts of csrc/i2c_quad.hpp, mirrored in quad_eligible), no default batch window;
  * straight-line bodies: `const R tN = ...;` temporaries of sympy.cse, constants with all 17 significant digits, r_rcp for a
    division by a non-constant, integer powers as products;
  * optionally `jacobian<FN, R>()`: value and Jacobian of one function with their common subexpressions shared, which
    value_and_jacobian (csrc/i2c_linearize.hpp) calls instead of d + 1 dual-number passes.
A model that states `operations = "extended"` (TracedModel.operations; trace(..., operations="extended")) may also use sqrt,
tanh, log, abs, minimum, maximum, where_gt(a, b, x, y), Python's abs() and half-integer powers, and take the sine of anything: a
sine whose argument is an integer combination of STATE inputs plus a constant stays an angle coordinate, any other argument (a
product, a parameter, an action, a nested function) is a GENERAL sine, emitted as one r_sincos call per distinct argument and
function body, its sine, cosine and derivatives sharing the pair. The derivative conventions of the new nodes are those of the
dual-number overloads (csrc/i2c_linearize.hpp): abs' = sign (0 at 0), min / max take the first argument's derivative at a tie,
where_gt the selected branch's, and the tangent of a half-integer power goes through r_tangent (a zero tangent stays zero at 0).
A basic model traces, refuses and emits exactly as before the wider set existed.
sympy is imported when the first model is traced, never on import of this module.
"""
import hashlib
import os
import re
import threading
import types

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
GEN_DIR = os.path.join(PKG_DIR, "lib", "generated")

FUNCTIONS = ("dynamics", "observe", "observe_terminal", "measure")
# ... and the OPTIONAL fifth: the state-action-dependent part Q(xu) of the one-step covariance, sym(NX) packed-lower expressions of the
# dynamics' inputs (the functor's optional process_noise member, csrc/i2c_cell.hpp). Traced only when the model gives it, with the
# same operation sets and refusals; no Jacobian is emitted for it. A model without it emits the text it always did.
PROCESS_NOISE = "process_noise"

OPERATIONS = "sin, cos, exp, clip(x, lo, hi), rcp, pi and + - * / with integer powers"
OPERATIONS_EXTENDED = ("sin, cos, exp, sqrt, tanh, log, abs, minimum, maximum, where_gt(a, b, x, y), clip(x, lo, hi), rcp, pi and "
                       "+ - * / with integer and half-integer powers")
HINT = ' (a model that sets operations = "extended" may use it)'
# capacities of the host constants in I2cProblem (checked at registration) and of the one-lane kernels (d <= 8)
LIMITS = {"d": 8, "NX": 12, "NU": 4, "NZ": 16, "NZT": 16, "NY": 16, "NP": 16}
INT_KNOBS = ("GROUP", "QUAD_FORWARD_MAX_B", "QUAD_FORWARD_MIN_B", "QUAD_BACKWARD8_MIN_B", "QUAD_BACKWARD8_MAX_B",
             "QUAD_CHUNK_WALK_MIN_B", "QUAD_CHUNK_WALK_MAX_B", "QUAD_CHUNK_PASSES_MIN_B", "QUAD_CHUNK_PASSES_MAX_B",
             "QUAD_CHUNK_STITCH_MAX_B", "BWD_FUSED_MIN_B")
BOOL_KNOBS = ("QUAD", "GROUP_FORWARD_AUTO")

_ENV = None
_ENV_LOCK = threading.Lock()


def pack_lower(out, nx):
    """sym(nx) packed-lower (row-major) entries from what a process_noise function returned: those entries themselves, or the full
    nx x nx matrix as nx rows (lists or tuples of nx entries each), whose lower triangle is taken. Only the matrix form is recognised
    here -- for nx = 1 that is `[[q]]`, while `[q]` is the packed form --; anything else is passed on as it is, and a wrong number
    of entries (three flat entries for nx = 3, say) is refused by the caller's count check like any other function's."""
    out = list(out)
    if len(out) == nx and all(isinstance(r, (list, tuple)) and len(r) == nx for r in out):
        return [out[i][j] for i in range(nx) for j in range(i + 1)]
    return out


def _env():
    """sympy and the two function symbols of clip, created on first use (once: expressions are recognised by these classes)."""
    global _ENV
    with _ENV_LOCK:
        if _ENV is None:
            _ENV = _make_env()
    return _ENV


def _make_env():
    import sympy as sp

    class ClipInside(sp.Function):
        """1 strictly inside the limits, 0 on and outside them: autograd's derivative of clip (r_clip(Dual), i2c_linearize.hpp)."""
        nargs = 3

    class Clip(sp.Function):
        nargs = 3

        def fdiff(self, argindex=1):
            return ClipInside(*self.args) if argindex == 1 else sp.S.Zero

    class WhereGt(sp.Function):
        """where_gt(a, b, x, y) = x if a > b else y; the derivative of the selected branch, nothing through a or b."""
        nargs = 4

        def fdiff(self, argindex=1):
            a, b = self.args[:2]
            return WhereGt(a, b, sp.S.One, sp.S.Zero) if argindex == 3 else WhereGt(a, b, sp.S.Zero, sp.S.One) if argindex == 4 else sp.S.Zero

    class Max2(sp.Function):
        """r_max(a, b) = b if b > a else a: at a tie the first argument, and its derivative."""
        nargs = 2

        def fdiff(self, argindex=1):
            a, b = self.args
            return WhereGt(b, a, sp.S.Zero, sp.S.One) if argindex == 1 else WhereGt(b, a, sp.S.One, sp.S.Zero)

    class Min2(sp.Function):
        """r_min(a, b) = b if b < a else a."""
        nargs = 2

        def fdiff(self, argindex=1):
            a, b = self.args
            return WhereGt(a, b, sp.S.Zero, sp.S.One) if argindex == 1 else WhereGt(a, b, sp.S.One, sp.S.Zero)

    class SignF(sp.Function):
        """1, -1, and 0 at 0: the derivative of abs (r_sign)."""
        nargs = 1

        def fdiff(self, argindex=1):
            return sp.S.Zero

    class AbsF(sp.Function):
        nargs = 1

        def fdiff(self, argindex=1):
            return SignF(self.args[0])

    class GSin(sp.Function):
        """The sine of a general argument: one half of an r_sincos pair (GCos the other)."""
        nargs = 1

        def fdiff(self, argindex=1):
            return GCos(self.args[0])

    class GCos(sp.Function):
        nargs = 1

        def fdiff(self, argindex=1):
            return -GSin(self.args[0])

    class SqrtGrad(sp.Function):
        """rsqrt(x) / 2, +inf at 0 (r_sqrt_grad)."""
        nargs = 1

    class Tangent(sp.Function):
        """g * d with a zero tangent d kept exactly zero (r_tangent)."""
        nargs = 2

    class SymMath:
        """The operation set of a functor, on sympy expressions."""
        pi = sp.pi
        sin, cos, exp = staticmethod(sp.sin), staticmethod(sp.cos), staticmethod(sp.exp)

        @staticmethod
        def clip(x, lo, hi):
            return Clip(sp.sympify(x), sp.sympify(lo), sp.sympify(hi))

        @staticmethod
        def rcp(x):
            return 1 / sp.sympify(x)

        def __getattr__(self, name):
            hint = HINT if name in ("sqrt", "tanh", "log", "abs", "minimum", "maximum", "where_gt") else ""
            raise ValueError(f"m.{name} is outside the operation set of a device functor ({OPERATIONS}){hint}")

    class SymMathExtended(SymMath):
        """... of a model with operations = "extended"."""
        sqrt, tanh, log, abs = staticmethod(sp.sqrt), staticmethod(sp.tanh), staticmethod(sp.log), staticmethod(sp.Abs)

        @staticmethod
        def minimum(a, b):
            return Min2(sp.sympify(a), sp.sympify(b))

        @staticmethod
        def maximum(a, b):
            return Max2(sp.sympify(a), sp.sympify(b))

        @staticmethod
        def where_gt(a, b, x, y):
            return WhereGt(*(sp.sympify(v) for v in (a, b, x, y)))

        def __getattr__(self, name):
            raise ValueError(f"m.{name} is outside the operation set of a device functor ({OPERATIONS_EXTENDED})")

    return types.SimpleNamespace(sp=sp, Clip=Clip, ClipInside=ClipInside, math=SymMath(), math_extended=SymMathExtended(),
                                 WhereGt=WhereGt, Max2=Max2, Min2=Min2, SignF=SignF, AbsF=AbsF, GSin=GSin, GCos=GCos,
                                 SqrtGrad=SqrtGrad, Tangent=Tangent)


def sym_math(operations="basic"):
    return _env().math_extended if operations == "extended" else _env().math


class Spec:
    """What trace() found: dims, the expressions of every function over the symbols xu / p / sn / cs, and the angle inputs."""

    def __init__(self, dims, n_params):
        self.NX, self.NU, self.NZ, self.NZT, self.NY = (int(dims[k]) for k in ("NX", "NU", "NZ", "NZT", "NY"))
        self.NP = int(n_params)
        self.D = self.NX + self.NU
        self.exprs = {}   # function -> [expression per output]
        self.angles = []  # input index of angle a
        self.extended = False    # operations = "extended"
        self.general_sines = []  # the distinct arguments of the general sines (extended models), over all functions

    def n_in(self, fn):
        return self.D if fn in ("dynamics", "observe", PROCESS_NOISE) else self.NX

    def n_out(self, fn):
        return {"dynamics": self.NX, "observe": self.NZ, "observe_terminal": self.NZT, "measure": self.NY,
                PROCESS_NOISE: self.NX * (self.NX + 1) // 2}[fn]


def check_limits(dims, n_params, who="model"):
    d = dims["NX"] + dims["NU"]
    sizes = dict(dims, d=d, NP=n_params)
    for key, cap in LIMITS.items():
        if sizes[key] > cap:
            raise ValueError(f"{who}: {key} = {sizes[key]} exceeds {cap}, the most a traced model may have (d <= 8: the one-lane kernels; "
                             "NX <= 12, NU <= 4, NZ, NZT, NY, NP <= 16: the host constants of I2cProblem). Larger models take the header "
                             "route: a hand-written functor with GROUP_ONLY (INTEGRATION.md section 3)")
    if dims["NX"] < 1 or dims["NU"] < 1 or dims["NZ"] < 1:
        raise ValueError(f"{who}: dim_x, dim_u and dim_z must be at least 1")


def trace(dims, fns, n_params, who="model", operations="basic"):
    """dims: {"NX", "NU", "NZ", "NZT", "NY"}; fns: {function name: callable(inputs, p, m)}; -> Spec."""
    if operations not in ("basic", "extended"):
        raise ValueError(f"{who}: operations = {operations!r}; a traced model states \"basic\" or \"extended\"")
    check_limits(dims, n_params, who)
    env = _env()
    sp = env.sp
    spec = Spec(dims, n_params)
    ext = spec.extended = operations == "extended"
    ops = OPERATIONS_EXTENDED if ext else OPERATIONS
    xs = [sp.Symbol(f"xu{i}", real=True) for i in range(spec.D)]
    ps = [sp.Symbol(f"p{i}", real=True) for i in range(spec.NP)]
    spec.xs, spec.ps = xs, ps
    raw = {}
    functions = spec.functions = FUNCTIONS + ((PROCESS_NOISE,) if fns.get(PROCESS_NOISE) is not None else ())
    for fn in functions:
        label = f"{who}.{fn}_fn"
        n_in, n_out = spec.n_in(fn), spec.n_out(fn)
        try:
            out = fns[fn](list(xs[:n_in]), list(ps), env.math_extended if ext else env.math)
            out = [] if out is None else list(out)
            if fn == PROCESS_NOISE:
                out = pack_lower(out, spec.NX)
        except (TypeError, AttributeError) as e:
            raise ValueError(f"{label}: {e} -- a Python branch, comparison or foreign function on a traced value cannot be compiled "
                             f"(the operation set is {ops})") from e
        except ValueError as e:
            raise ValueError(f"{label}: {e}") from e
        if len(out) != n_out:
            raise ValueError(f"{label} returned {len(out)} expressions where the model states {n_out}")
        try:
            raw[fn] = [sp.sympify(o) for o in out]
        except (sp.SympifyError, TypeError) as e:
            raise ValueError(f"{label}: an output is not an expression of the inputs: {e}") from e
    # angles: every sine / cosine brought to sin(xu_j) / cos(xu_j)
    ang = set()
    normal = {}
    general = set()
    for fn in functions:
        if ext:  # (state inputs only: a sine of anything else is a general sine, not an error)
            normal[fn] = [_split_sines(_normalise(e), xs[:min(spec.n_in(fn), spec.NX)], ang, general) for e in raw[fn]]
        else:
            normal[fn] = [_expand_angles(e, xs[:spec.n_in(fn)], f"{who}.{fn}_fn", k, ang) for k, e in enumerate(raw[fn])]
    spec.angles = sorted(ang)
    if spec.angles and spec.angles[-1] >= spec.NX:
        raise ValueError(f"{who}: the sine / cosine of action input {spec.angles[-1]} occurs; angle coordinates must be states "
                         "(the terminal functions receive the sines of the state alone)")
    spec.sn = [sp.Symbol(f"sn{a}", real=True) for a in range(len(spec.angles))]
    spec.cs = [sp.Symbol(f"cs{a}", real=True) for a in range(len(spec.angles))]
    table = {}
    for a, j in enumerate(spec.angles):
        table[sp.sin(xs[j])] = spec.sn[a]
        table[sp.cos(xs[j])] = spec.cs[a]
    allowed = set(xs) | set(ps) | set(spec.sn) | set(spec.cs)
    for fn in functions:
        spec.exprs[fn] = [e.xreplace(table) for e in normal[fn]]
        for k, e in enumerate(spec.exprs[fn]):
            _check_operations(e, allowed, f"{who}.{fn}_fn", k, ext)
    spec.general_sines = sorted((a.xreplace(table) for a in general), key=sp.default_sort_key)
    return spec


def _normalise(expr):
    """Extended models: abs() as the node with the derivative convention, and a floating-point exponent that is an integer or a
    half-integer (x ** 0.5, x ** -1.5, x ** 2.0) as that rational."""
    env = _env()
    sp = env.sp

    def exponent(e):
        return e.is_Pow and e.exp.is_Float and float(2 * e.exp) == int(float(2 * e.exp))

    expr = expr.replace(exponent, lambda e: sp.Pow(e.base, sp.Rational(int(float(2 * e.exp)), 2)))
    return expr.replace(sp.Abs, env.AbsF)


def _split_sines(expr, states, ang, general):
    """Extended models, bottom-up: a sine / cosine of an integer combination of state inputs plus a constant becomes sines and
    cosines of single states (angle addition; the states join `ang`), any other one a general sine (its argument joins `general`)."""
    env = _env()
    sp = env.sp
    if expr.is_Atom:
        return expr
    args = [_split_sines(a, states, ang, general) for a in expr.args]
    if any(a is not b for a, b in zip(args, expr.args)):
        expr = expr.func(*args)
    if not isinstance(expr, (sp.sin, sp.cos)):
        return expr
    arg, new_arg = sp.expand(expr.args[0]), sp.S.Zero
    for term, coeff in arg.as_coefficients_dict().items():
        if term == 1 or (term.is_number and not term.free_symbols):
            new_arg += coeff * term
        elif term in states and coeff.is_number and float(coeff) == int(float(coeff)):
            new_arg += sp.Integer(int(float(coeff))) * term
        else:
            new_arg = None
            break
    if new_arg is not None and not new_arg.atoms(sp.Function):
        new = sp.expand_trig(expr.func(new_arg))
        if all(s.args[0] in states for s in new.atoms(sp.sin, sp.cos)):
            ang.update(states.index(s.args[0]) for s in new.atoms(sp.sin, sp.cos))
            return new
    general.add(expr.args[0])
    return (env.GSin if isinstance(expr, sp.sin) else env.GCos)(expr.args[0])


def _expand_angles(expr, inputs, label, k, ang):
    sp = _env().sp
    table = {}
    for t in expr.atoms(sp.sin, sp.cos):
        name = t.func.__name__
        arg = sp.expand(t.args[0])
        new_arg = sp.S.Zero
        for term, coeff in arg.as_coefficients_dict().items():
            if term == 1 or (term.is_number and not term.free_symbols):
                new_arg += coeff * term
            elif term in inputs and coeff.is_number and float(coeff) == int(float(coeff)):
                new_arg += sp.Integer(int(float(coeff))) * term
            else:
                raise ValueError(f"{label}: output {k}: the argument of {name}({t.args[0]}) is not an integer combination of inputs plus "
                                 f"a constant (term '{coeff * term}'): a functor is handed sin / cos of its angle coordinates and may not "
                                 "call a sine itself")
        new = sp.expand_trig(t.func(new_arg))
        for s in new.atoms(sp.sin, sp.cos):
            if s.args[0] not in inputs:
                raise ValueError(f"{label}: output {k}: {name}({t.args[0]}) does not reduce to sines and cosines of single inputs "
                                 f"(left with {s})")
            ang.add(inputs.index(s.args[0]))
        table[t] = new
    return expr.xreplace(table) if table else expr


def _check_operations(e, allowed, label, k, ext=False):
    env = _env()
    sp = env.sp
    ops = OPERATIONS_EXTENDED if ext else OPERATIONS
    if e in allowed:
        return
    if not e.free_symbols and e.is_number and not e.atoms(sp.Function):
        if e.has(sp.zoo, sp.oo, -sp.oo, sp.nan) or not e.is_real:
            raise ValueError(f"{label}: output {k}: the constant {e} is not a finite real number")
        return
    if e.is_Add or e.is_Mul:
        for a in e.args:
            _check_operations(a, allowed, label, k, ext)
        return
    if e.is_Pow:
        half = e.exp.is_Rational and e.exp.q == 2 or e.exp.is_Float and float(2 * e.exp) == int(float(2 * e.exp))
        if ext and e.exp.is_Rational and e.exp.q == 2:
            return _check_operations(e.base, allowed, label, k, ext)
        if not e.exp.is_Integer:
            raise ValueError(f"{label}: output {k}: the power {e} has a non-integer exponent, which is outside the operation set "
                             f"({ops})" + (HINT if half and not ext else ""))
        return _check_operations(e.base, allowed, label, k, ext)
    if isinstance(e, (sp.exp, env.Clip, env.ClipInside)) or ext and isinstance(
            e, (sp.tanh, sp.log, env.AbsF, env.SignF, env.Min2, env.Max2, env.WhereGt, env.GSin, env.GCos)):
        for a in e.args:
            _check_operations(a, allowed, label, k, ext)
        return
    what = e.func.__name__ if hasattr(e.func, "__name__") else str(e.func)
    raise ValueError(f"{label}: output {k}: '{what}' in {e} is outside the operation set of a device functor ({ops})"
                     + (HINT if what in ("Abs", "tanh", "log") and not ext else ""))


# ---- structure hints and family knobs -------------------------------------------------------------------------------------------
def hints(spec, fn):
    """(lin, dep) per output: lin[k] = j where output k is literally input j (else -1); dep[k] = the largest input index the output
    depends on (a pass-through: its own input)."""
    xs = spec.xs
    via = {s: spec.angles[a] for a, s in enumerate(spec.sn)}
    via.update({c: spec.angles[a] for a, c in enumerate(spec.cs)})
    lin, dep = [], []
    for e in spec.exprs[fn]:
        lin.append(xs.index(e) if e in xs else -1)
        idx = [xs.index(s) if s in xs else via[s] for s in e.free_symbols if s in xs or s in via]
        dep.append(max(idx) if idx else 0)
    return lin, dep


def default_group(spec):
    """The narrowest group with a matrix row per lane: G >= d, nz, nzt, ny (the static_asserts of csrc/i2c_group.hpp)."""
    need = max(spec.D, spec.NZ, spec.NZT, spec.NY)
    return next(g for g in (4, 8, 16) if g >= need)


def quad_eligible(spec):
    """Whether the d <= 8 quad kernels instantiate on the model: the static_asserts of forward_quad_body and q_points
    (csrc/i2c_quad.hpp). The backward walk and the chunk passes are gated by quad_backward8_exists and need no knob."""
    NX, NU, NZ, NZT, D = spec.NX, spec.NU, spec.NZ, spec.NZT, spec.D
    obs_lin, term_lin = hints(spec, "observe")[0], hints(spec, "observe_terminal")[0]
    obs_id = NZ == D and all(obs_lin[k] == k for k in range(NZ))           # OBS_ID
    term_id = NZT == NX and all(term_lin[k] == k for k in range(NZT))      # TERM_ID
    if D > 8:                                          # QG<M>::WIDE: the d = 16 geometry, another set of conditions
        return False
    if not obs_id and (D % 4 == 0 or NU != 1):         # "a spare column in the joint's last block", "one action"
        return False
    if NX % 4 + NU > 4:                                # "the action entries live in one block"
        return False
    if (NZ + 3) // 4 > NX * (NX + 1) // 2:             # "dummy rows of the target prefetch"
        return False
    jzl = obs_lin[NZ - 1]
    lastlin = not obs_id and NZ % 4 == 1 and NZ > 4 and jzl >= 0 and jzl // 4 == (D + 3) // 4 - 1  # LASTLIN: the last output is not evaluated
    if not obs_id and NZ - (1 if lastlin else 0) > 12:  # q_points: "<= 12 evaluated outputs"
        return False
    if NZT > 0 and not term_id and NZT > 12:
        return False
    return True


# ---- C++ ------------------------------------------------------------------------------------------------------------------------
def literal(v):
    v = float(v)
    if v != v or v in (float("inf"), float("-inf")):
        raise ValueError(f"constant {v} cannot be written into a functor")
    return f"R({v!r})"


class _Printer:
    def __init__(self, names):
        self.names = dict(names)
        self.env = _env()

    def atom(self, e):
        """e as an operand of * or unary minus"""
        s = self.expr(e)
        return f"({s})" if e.is_Add or (e.is_Mul and s.startswith("-")) else s

    def expr(self, e):
        sp, env = self.env.sp, self.env
        if e in self.names:
            return self.names[e]
        if not e.free_symbols and e.is_number and not e.atoms(sp.Function):
            return literal(sp.N(e, 30))
        if e.is_Add:
            pos, neg = [], []
            for t in e.args:
                c, _ = t.as_coeff_Mul()
                (neg if c.is_negative else pos).append(t)
            out = " + ".join(self.term(t) for t in pos)
            if not pos:
                out = "-" + self.atom(-neg[0])
                neg = neg[1:]
            for t in neg:
                out += " - " + self.term(-t)
            return out
        if e.is_Mul:
            return self.term(e)
        if e.is_Pow and e.exp.is_Rational and e.exp.q == 2:  # b^(n/2), n odd: b^((n - 1) / 2) r_sqrt(b) or r_rsqrt(b)^|n|
            n, b = int(e.exp.p), self.expr(e.base)
            if n < 0:
                return " * ".join([f"r_rsqrt({b})"] * -n)
            lead = self.atom(e.base) if not (e.base.is_Mul or e.base.is_Pow) else f"({b})"
            return " * ".join([lead] * ((n - 1) // 2) + [f"r_sqrt({b})"])
        if e.is_Pow:
            n = int(e.exp)
            b = self.atom(e.base) if not (e.base.is_Mul or e.base.is_Pow) else f"({self.expr(e.base)})"
            prod = " * ".join([b] * abs(n))
            return prod if n > 0 else f"r_rcp({prod})"
        if isinstance(e, sp.exp):
            return f"r_exp({self.expr(e.args[0])})"
        if isinstance(e, env.Clip):
            return "r_clip(" + ", ".join(self.typed(a) for a in e.args) + ")"
        if isinstance(e, env.ClipInside):
            return "r_clip_grad(" + ", ".join(self.typed(a) for a in e.args) + ")"
        for cls, fn in ((sp.tanh, "r_tanh"), (sp.log, "r_log"), (env.AbsF, "r_abs"), (env.SignF, "r_sign"), (env.Min2, "r_min"),
                        (env.Max2, "r_max"), (env.WhereGt, "r_where_gt"), (env.SqrtGrad, "r_sqrt_grad"), (env.Tangent, "r_tangent")):
            if isinstance(e, cls):
                return f"{fn}(" + ", ".join(self.typed(a) for a in e.args) + ")"
        raise ValueError(f"cannot print {e}")

    def typed(self, e):
        """an argument of a function template: an expression of type R whatever it is made of"""
        s = self.expr(e)
        return s if e in self.names or s.startswith("R(") and s.count("(") == 1 else f"R({s})"

    def term(self, e):
        """a product: [-] [constant *] numerator factors [* r_rcp(denominator factors)]"""
        c, rest = e.as_coeff_Mul()
        num, den = [], []
        for f in self.env.sp.Mul.make_args(rest):
            if f.is_Pow and f.exp.is_Integer and f.exp.is_negative and f.base.free_symbols:
                den.append(f.base ** (-f.exp))
            elif f != 1:
                num.append(f)
        sign = "-" if c.is_negative else ""
        c = abs(c)
        parts = ([literal(self.env.sp.N(c, 30))] if c != 1 else []) + [self.factor(f) for f in num]
        if den:
            parts.append("r_rcp(" + " * ".join(self.factor(f) for f in den) + ")")
        if not parts:
            parts = [literal(1.0)]
        return sign + " * ".join(parts)

    def factor(self, f):
        if f.is_Pow and f.exp.is_Integer and f.exp.is_positive:
            return self.expr(f)
        return self.atom(f)


def _body(names, defs, outs, indent="    "):
    """Straight-line code for `defs` [(symbol, expression)] and `outs` [(target, expression)]: one sympy.cse over all of them, every
    temporary as `const R name = ...;` in dependency order, then `target = expression;` for every output."""
    env = _env()
    sp = env.sp
    if not outs:
        return ""
    # general sines (extended models): every distinct argument is one pair (gN, hN) = r_sincos(argument), innermost first
    pairs, defs, outs = {}, list(defs), list(outs)
    while True:
        nodes = set().union(*[e.atoms(env.GSin, env.GCos) for _, e in defs + outs])
        args = sorted({n.args[0] for n in nodes if not n.args[0].atoms(env.GSin, env.GCos)}, key=sp.default_sort_key)
        if not args:
            break
        table = {}
        for a in args:
            g, h = sp.Symbol(f"g{len(pairs)}", real=True), sp.Symbol(f"h{len(pairs)}", real=True)
            pairs[g] = h
            defs.append((g, a))  # (the definition of g stands for the pair's call: see below)
            table[env.GSin(a)], table[env.GCos(a)] = g, h
        defs = [(s, e if s in table.values() else e.xreplace(table)) for s, e in defs]
        outs = [(t, e.xreplace(table)) for t, e in outs]
    repl, reduced = sp.cse([e for _, e in defs] + [e for _, e in outs], symbols=sp.numbered_symbols("t"), order="canonical")
    pending = list(repl) + [(s, reduced[i]) for i, (s, _) in enumerate(defs)]
    pr = _Printer(names)
    known = set(names)
    lines = []
    while pending:
        later = []
        for sym, e in pending:
            if e.free_symbols <= known and sym in pairs:
                lines.append(f"{indent}R {sym}, {pairs[sym]};\n{indent}r_sincos({pr.typed(e)}, &{sym}, &{pairs[sym]});")
                for v in (sym, pairs[sym]):
                    known.add(v)
                    pr.names[v] = str(v)
            elif e.free_symbols <= known:
                lines.append(f"{indent}const R {sym} = {pr.typed(e) if not e.free_symbols else pr.expr(e)};")
                known.add(sym)
                pr.names[sym] = str(sym)
            else:
                later.append((sym, e))
        assert len(later) < len(pending), "cyclic temporaries"
        pending = later
    for (tgt, _), e in zip(outs, reduced[len(defs):]):
        lines.append(f"{indent}{tgt} = {pr.typed(e) if not e.free_symbols else pr.expr(e)};")
    return "\n".join(lines) + "\n"


def _names(spec, n_in):
    names = {s: f"x[{i}]" for i, s in enumerate(spec.xs[:n_in])}
    names.update({s: f"p[{i}]" for i, s in enumerate(spec.ps)})
    names.update({s: f"sn[{a}]" for a, s in enumerate(spec.sn)})
    names.update({s: f"cs[{a}]" for a, s in enumerate(spec.cs)})
    return names


def jacobian_program(spec, fn):
    """Value and Jacobian of one function by forward-mode differentiation of its expression GRAPH: the values are split into
    temporaries first (sympy.cse), then every temporary gets its derivative with respect to every input from the derivatives of
    what it is made of -- the chain rule the dual numbers apply, written out once with the zero terms dropped. (Differentiating
    the whole expression of an output instead swells it, and rounds further from the dual-number path.) The sines are functions
    of their inputs: d sn_a = cs_a, d cs_a = -sn_a where ang(a) = j. -> (defs [(symbol, expression)], values, jacobian row-major)"""
    env = _env()
    sp = env.sp
    n_in = spec.n_in(fn)
    zero, one = sp.S.Zero, sp.S.One
    grad = {x: [one if i == j else zero for j in range(n_in)] for i, x in enumerate(spec.xs[:n_in])}
    for a, ja in enumerate(spec.angles):
        grad[spec.sn[a]] = [spec.cs[a] if j == ja else zero for j in range(n_in)]
        grad[spec.cs[a]] = [-spec.sn[a] if j == ja else zero for j in range(n_in)]

    def derivative(e, j):
        # (extended models) the outermost half-integer powers are differentiated as symbols of their own, whose tangent goes
        # through r_tangent: a zero tangent stays exactly zero where the factor rsqrt(base) is infinite
        halves = sorted((q for q in e.atoms(sp.Pow) if q.exp.is_Rational and q.exp.q == 2), key=sp.default_sort_key) if spec.extended else []
        halves = [q for q in halves if not any(o is not q and o.base.has(q) for o in halves)]
        lift, tangent = {}, {}
        for i, q in enumerate(halves):
            w, db = sp.Dummy(f"w{i}", real=True), derivative(q.base, j)
            factor = env.SqrtGrad(q.base) if q.exp == sp.Rational(1, 2) else q.exp * sp.Pow(q.base, q.exp - 1)
            lift[q], tangent[w] = w, (env.Tangent(factor, db) if db != 0 else zero)
        if lift:
            e = e.xreplace(lift)
        d = sp.Add(*[sp.diff(e, s) * (tangent[s] if s in tangent else grad[s][j]) for s in e.free_symbols
                     if (tangent[s] if s in tangent else grad[s][j] if s in grad else zero) != 0])
        return d.xreplace({w: q for q, w in lift.items()}) if lift else d

    repl, values = sp.cse(list(spec.exprs[fn]), symbols=sp.numbered_symbols("v"), order="canonical")
    defs = []
    for sym, e in repl:
        defs.append((sym, e))
        grad[sym] = []
        for j in range(n_in):
            d = derivative(e, j)
            if d.free_symbols and not d.is_Symbol:
                dsym = sp.Symbol(f"d{sym}_{j}", real=True)
                defs.append((dsym, d))
                d = dsym
            grad[sym].append(d)
    return defs, values, [derivative(e, j) for e in values for j in range(n_in)]


def _select(name, values, default, arg="k"):
    """`int name(int k)` as a chain of conditionals over the outputs (constant-folds after unrolling)."""
    if not values:
        return f"  I2C_HD static constexpr int {name}(int) {{ return {default}; }}\n"
    if len(set(values)) == 1:
        return f"  I2C_HD static constexpr int {name}(int) {{ return {values[0]}; }}\n"
    chain = " : ".join(f"{arg} == {k} ? {v}" for k, v in enumerate(values[:-1])) + f" : {values[-1]}"
    return f"  I2C_HD static constexpr int {name}(int {arg}) {{ return {chain}; }}\n"


def resolve_knobs(spec, knobs=None):
    out = {"GROUP": default_group(spec), "QUAD": quad_eligible(spec)}
    for key, v in (knobs or {}).items():
        if key not in INT_KNOBS + BOOL_KNOBS:
            raise ValueError(f"unknown knob '{key}'; a traced model may set {', '.join(BOOL_KNOBS + INT_KNOBS)}")
        out[key] = bool(v) if key in BOOL_KNOBS else int(v)
    return out


def emit(spec, struct, jacobian=True, knobs=None, origin=None):
    """The text of the header: struct `struct` in namespace i2c, derived from ModelDefaults, laid out as INTEGRATION.md section 3."""
    if not re.fullmatch(r"[A-Za-z_][A-Za-z0-9_]*", struct):
        raise ValueError(f"'{struct}' is not a C++ identifier")
    kn = resolve_knobs(spec, knobs)
    s = [f"// Device functor of {origin or struct}, generated by functor_codegen.py from the model's Python functions (INTEGRATION.md\n"
         "// section 3b). Do not edit: change the Python class; the file name carries a hash of this text.\n"
         "#pragma once\n\nnamespace i2c {\n\n"
         f"struct {struct} : ModelDefaults {{\n"
         f"  static constexpr int NX = {spec.NX}, NU = {spec.NU}, NZ = {spec.NZ}, NZT = {spec.NZT}, NP = {spec.NP}, "
         f"NA = {len(spec.angles)}, NY = {spec.NY};\n"]
    for key, v in kn.items():
        s.append(f"  static constexpr {'bool' if key in BOOL_KNOBS else 'int'} {key} = {str(v).lower() if key in BOOL_KNOBS else v};\n")
    s.append(_select("ang", spec.angles, 0, arg="a"))
    for fn, stem in (("observe", "obs"), ("observe_terminal", "term"), ("measure", "meas")):
        lin, dep = hints(spec, fn)
        s.append(_select(f"{stem}_lin", lin, -1))
        s.append(_select(f"{stem}_dep", dep, 0))
    for fn in FUNCTIONS:
        n_in = spec.n_in(fn)
        body = _body(_names(spec, n_in), [], [(f"y[{k}]", e) for k, e in enumerate(spec.exprs[fn])])
        s.append(f"  template <typename R> I2C_FN void {fn}(const R* p, const R* x, const R* sn, const R* cs, R* y) {{\n{body}  }}\n")
    if PROCESS_NOISE in spec.exprs:
        body = _body(_names(spec, spec.D), [], [(f"q[{k}]", e) for k, e in enumerate(spec.exprs[PROCESS_NOISE])])
        s.append("  // the state-action-dependent part of the one-step covariance at the point x = (state, action): q[sym(NX)], packed lower\n"
                 f"  template <typename R> I2C_FN void {PROCESS_NOISE}(const R* p, const R* x, const R* sn, const R* cs, R* q) {{\n{body}  }}\n")
    if jacobian:
        s.append("  // value and Jacobian of one function (FN: 0 dynamics, 1 observe, 2 observe_terminal), Jac[k * DIN + j] = d y_k / d x_j\n"
                 "  template <int FN, typename R> I2C_FN void jacobian(const R* p, const R* x, const R* sn, const R* cs, R* y, R* Jac) {\n")
        for i, fn in enumerate(FUNCTIONS[:3]):
            n_in, n_out = spec.n_in(fn), spec.n_out(fn)
            defs, values, jac = jacobian_program(spec, fn)
            targets = [f"y[{k}]" for k in range(n_out)] + [f"Jac[{k * n_in + j}]" for k in range(n_out) for j in range(n_in)]
            body = _body(_names(spec, n_in), defs, list(zip(targets, values + jac)), indent="      ")
            s.append(f"    {'if' if i == 0 else '} else if'} constexpr (FN == {i}) {{\n{body}")
        s.append("    }\n  }\n")
    s.append("};\n\n}  // namespace i2c\n")
    return "".join(s)


def snake(name):
    return re.sub(r"(?<=[a-z0-9])(?=[A-Z])", "_", name).lower()


def emit_unique(spec, base, **kw):
    """-> (text, struct, stem): the header with a struct name that carries a hash of the text, `<base>_<hash>`, and the file / library
    stem `<base in snake case>_<hash>`. Two versions of a model are then two C++ types: loaded into one process they share no
    template instantiation (same-named structs with different bodies would, through vague linkage), and a changed model is another
    library."""
    text = emit(spec, base, **kw)
    h = hashlib.sha256(text.encode()).hexdigest()[:12]
    struct, head = f"{base}_{h}", f"struct {base} : ModelDefaults"
    assert text.count(head) == 1
    return text.replace(head, f"struct {struct} : ModelDefaults"), struct, f"{snake(base)}_{h}"


def write_header(text, stem, out_dir=None):
    """-> path of <stem>.hpp. An unchanged header keeps its file -- and its modification time, by which build.build_model decides
    whether to rebuild."""
    out_dir = out_dir or GEN_DIR
    path = os.path.join(out_dir, stem + ".hpp")
    old = None
    if os.path.exists(path):
        with open(path) as f:
            old = f.read()
    if old != text:
        os.makedirs(out_dir, exist_ok=True)
        tmp = f"{path}.{os.getpid()}.tmp"
        with open(tmp, "w") as f:
            f.write(text)
        os.replace(tmp, path)
    return path
