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
OPERATIONS = "sin, cos, exp, clip(x, lo, hi), rcp, pi and + - * / with integer powers"
# capacities of the host constants in I2cProblem (checked at registration) and of the one-lane kernels (d <= 8)
LIMITS = {"d": 8, "NX": 12, "NU": 4, "NZ": 16, "NZT": 16, "NY": 16, "NP": 16}
INT_KNOBS = ("GROUP", "QUAD_FORWARD_MAX_B", "QUAD_FORWARD_MIN_B", "QUAD_BACKWARD8_MIN_B", "QUAD_BACKWARD8_MAX_B",
             "QUAD_CHUNK_WALK_MIN_B", "QUAD_CHUNK_WALK_MAX_B", "QUAD_CHUNK_PASSES_MIN_B", "QUAD_CHUNK_PASSES_MAX_B",
             "QUAD_CHUNK_STITCH_MAX_B", "BWD_FUSED_MIN_B")
BOOL_KNOBS = ("QUAD", "GROUP_FORWARD_AUTO")

_ENV = None
_ENV_LOCK = threading.Lock()


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
            raise ValueError(f"m.{name} is outside the operation set of a device functor ({OPERATIONS})")

    return types.SimpleNamespace(sp=sp, Clip=Clip, ClipInside=ClipInside, math=SymMath())


def sym_math():
    return _env().math


class Spec:
    """What trace() found: dims, the expressions of every function over the symbols xu / p / sn / cs, and the angle inputs."""

    def __init__(self, dims, n_params):
        self.NX, self.NU, self.NZ, self.NZT, self.NY = (int(dims[k]) for k in ("NX", "NU", "NZ", "NZT", "NY"))
        self.NP = int(n_params)
        self.D = self.NX + self.NU
        self.exprs = {}   # function -> [expression per output]
        self.angles = []  # input index of angle a

    def n_in(self, fn):
        return self.D if fn in ("dynamics", "observe") else self.NX

    def n_out(self, fn):
        return {"dynamics": self.NX, "observe": self.NZ, "observe_terminal": self.NZT, "measure": self.NY}[fn]


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


def trace(dims, fns, n_params, who="model"):
    """dims: {"NX", "NU", "NZ", "NZT", "NY"}; fns: {function name: callable(inputs, p, m)}; -> Spec."""
    check_limits(dims, n_params, who)
    env = _env()
    sp = env.sp
    spec = Spec(dims, n_params)
    xs = [sp.Symbol(f"xu{i}", real=True) for i in range(spec.D)]
    ps = [sp.Symbol(f"p{i}", real=True) for i in range(spec.NP)]
    spec.xs, spec.ps = xs, ps
    raw = {}
    for fn in FUNCTIONS:
        label = f"{who}.{fn}_fn"
        n_in, n_out = spec.n_in(fn), spec.n_out(fn)
        try:
            out = fns[fn](list(xs[:n_in]), list(ps), env.math)
            out = [] if out is None else list(out)
        except (TypeError, AttributeError) as e:
            raise ValueError(f"{label}: {e} -- a Python branch, comparison or foreign function on a traced value cannot be compiled "
                             f"(the operation set is {OPERATIONS})") from e
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
    for fn in FUNCTIONS:
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
    for fn in FUNCTIONS:
        spec.exprs[fn] = [e.xreplace(table) for e in normal[fn]]
        for k, e in enumerate(spec.exprs[fn]):
            _check_operations(e, allowed, f"{who}.{fn}_fn", k)
    return spec


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


def _check_operations(e, allowed, label, k):
    env = _env()
    sp = env.sp
    if e in allowed:
        return
    if not e.free_symbols and e.is_number and not e.atoms(sp.Function):
        if e.has(sp.zoo, sp.oo, -sp.oo, sp.nan) or not e.is_real:
            raise ValueError(f"{label}: output {k}: the constant {e} is not a finite real number")
        return
    if e.is_Add or e.is_Mul:
        for a in e.args:
            _check_operations(a, allowed, label, k)
        return
    if e.is_Pow:
        if not e.exp.is_Integer:
            raise ValueError(f"{label}: output {k}: the power {e} has a non-integer exponent, which is outside the operation set "
                             f"({OPERATIONS})")
        return _check_operations(e.base, allowed, label, k)
    if isinstance(e, (sp.exp, env.Clip, env.ClipInside)):
        for a in e.args:
            _check_operations(a, allowed, label, k)
        return
    what = e.func.__name__ if hasattr(e.func, "__name__") else str(e.func)
    raise ValueError(f"{label}: output {k}: '{what}' in {e} is outside the operation set of a device functor ({OPERATIONS})")


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
    sp = _env().sp
    if not outs:
        return ""
    repl, reduced = sp.cse([e for _, e in defs] + [e for _, e in outs], symbols=sp.numbered_symbols("t"), order="canonical")
    pending = list(repl) + [(s, reduced[i]) for i, (s, _) in enumerate(defs)]
    pr = _Printer(names)
    known = set(names)
    lines = []
    while pending:
        later = []
        for sym, e in pending:
            if e.free_symbols <= known:
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
    sp = _env().sp
    n_in = spec.n_in(fn)
    zero, one = sp.S.Zero, sp.S.One
    grad = {x: [one if i == j else zero for j in range(n_in)] for i, x in enumerate(spec.xs[:n_in])}
    for a, ja in enumerate(spec.angles):
        grad[spec.sn[a]] = [spec.cs[a] if j == ja else zero for j in range(n_in)]
        grad[spec.cs[a]] = [-spec.sn[a] if j == ja else zero for j in range(n_in)]

    def derivative(e, j):
        return sp.Add(*[sp.diff(e, s) * grad[s][j] for s in e.free_symbols if s in grad and grad[s][j] != 0])

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
