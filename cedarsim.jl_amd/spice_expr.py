"""SPICE numbers and expressions: `parse_number`, and `eval_expr` = tokenizer → precedence parser → `evaluate(tree, env)`.

A tree is nested tuples: `("num", v)`, `("name", n)`, `("call", n, args)`, `("neg" | "pos" | "not", x)`, `("and" | "or", a, b)`,
`("?", c, a, b)` and `(op, a, b)` for the operators of `_BINARY`.  The grammar, loosest first (it is what the earlier translation
to a Python source string gave in effect, and every expression that translation evaluated keeps its value bit for bit):

  1. `c ? a : b`, right-associative; only the chosen branch is evaluated
  2. `||`, then `&&`: both return the deciding operand (`2&&3` is 3.0, `0||3` is 3.0)
  3. prefix `!`, looser than comparison (`!a==b` is `!(a==b)`), so `1+!c` is an error and `1+(!c)` is not
  4. `== != < <= > >=`: one per level, `(a<b)<c` needs its parentheses
  5. `+ -`      6. `* /`      7. unary `+ -`
  8. `^` and `**`, right-associative, tighter than a sign on the left (`-2^2` is -4), a sign allowed on the right (`2**-1`)
  9. numbers with magnitudes (`1e3k`, `5v`), `name(args…)` from `_FUNCS`, dotted identifiers, `pi true false`, parentheses

An identifier found in `env` wins over a function or constant of the same name.  Values are Python floats, and truth values
Python bools until the final `float()`, combined with Python's own `/` and `**`; a complex result, a division by zero, a math
domain error and an overflow are a `CedarError`.  Every identifier must be defined, also in the branch of a ternary that is
not taken.

Deliberate differences from the translation to Python, which nothing else may join:
  * nested and parenthesised ternaries evaluate (they were syntax errors: the ternary was a textual split on the first `?`);
  * two accidents of Python's grammar are a `CedarError`: comparison chains (`a<b<1`) and floor division (`a//b`).
A comparison of random token strings with that translation found further spellings that evaluated only through Python's own
reading of the generated source.  No deck uses them, and they are errors too: a bare comma list read as a tuple (`min((1,2))`,
`c ? 1,2 : 3`, `!()`); `* *` with a blank read as `**`; two numerals in a row glued into one (`1k1a` was 1000.01e-18); a function
name before a parameter read as a call (`abs c`, `(sqrt)(4)`); an empty ternary branch (`c ? : 3`); and text that is no
expression behind an operand that `&&`, `||` or the ternary did not evaluate (`1 || a b`).  A `?` without its `:` raised
`ValueError`; it is a `CedarError` now.
"""
import decimal
import functools
import math
import operator
import re

from .circuit import CedarError

_MAG = {"t": "1e12", "g": "1e9", "meg": "1e6", "k": "1e3", "m": "1e-3", "u": "1e-6", "mil": "25.4e-6",
        "n": "1e-9", "p": "1e-12", "f": "1e-15", "a": "1e-18"}
_NUM_RE = re.compile(r"^([+-]?(?:\d+\.?\d*|\.\d+)(?:e[+-]?\d+)?)([a-z]*)$")


def parse_number(tok):
    """SPICE number with magnitude suffix → float, or None if not a number."""
    m = _NUM_RE.match(tok.strip().lower())
    if not m:
        return None
    num, suf = m.group(1), m.group(2)
    sf = None
    if suf:
        if suf.startswith("meg"):
            sf = _MAG["meg"]
        elif suf.startswith("mil"):
            sf = _MAG["mil"]
        elif suf[0] in _MAG:
            sf = _MAG[suf[0]]
        # otherwise: a pure unit such as "v" / "s" / "hz" — ignored
    d = decimal.Decimal(num)
    if sf is not None:
        d *= decimal.Decimal(sf)
    return float(d)


# ---- SPICE functions: src/spectre.jl source_body / test/basic.jl:651-684 ----
def _nint(x):
    return float(math.floor(x + 0.5)) if x >= 0 else float(-math.floor(-x + 0.5))


_FUNCS = {
    "sqrt": math.sqrt, "exp": math.exp, "ln": math.log, "log": math.log, "log10": math.log10, "abs": abs,
    "min": min, "max": max, "pow": math.pow, "pwr": lambda x, y: math.copysign(abs(x) ** y, x),
    "int": lambda x: float(math.trunc(x)), "nint": _nint, "floor": lambda x: float(math.floor(x)),
    "ceil": lambda x: float(math.ceil(x)), "sin": math.sin, "cos": math.cos, "tan": math.tan, "atan": math.atan,
    "sinh": math.sinh, "cosh": math.cosh, "tanh": math.tanh, "sgn": lambda x: float((x > 0) - (x < 0)),
    "pi": math.pi, "true": 1.0, "false": 0.0,
}
_TOKEN_RE = re.compile(r"\s*(?:(\d+\.?\d*(?:e[+-]?\d+)?[a-z]*|\.\d+(?:e[+-]?\d+)?[a-z]*)|([a-z_][a-z0-9_.]*)|(\*\*|&&|\|\||[<>=!]=|[-+*/^(),<>?:!]))", re.I)

_BINARY = {"==": operator.eq, "!=": operator.ne, "<": operator.lt, "<=": operator.le, ">": operator.gt, ">=": operator.ge,
           "+": operator.add, "-": operator.sub, "*": operator.mul, "/": operator.truediv, "**": operator.pow}
# left binding powers; a prefix `!` is allowed where the level asked for is no tighter than _NOT, a sign everywhere
_TERNARY, _OR, _AND, _NOT, _CMP, _SIGN = 1, 2, 3, 4, 5, 8
_LBP = {"?": _TERNARY, "||": _OR, "&&": _AND, "==": _CMP, "!=": _CMP, "<": _CMP, "<=": _CMP, ">": _CMP, ">=": _CMP,
        "+": 6, "-": 6, "*": 7, "/": 7, "**": 9}


class _Syntax(Exception):
    pass


def tokenize(s):
    """Lower-case expression text → (tokens, whole): tokens are `("num", value)`, `("name", identifier)` or `(operator,)` with `^`
    spelled `**`; `whole` is False when a character that starts no token ended the scan."""
    toks, pos = [], 0
    while pos < len(s):
        m = _TOKEN_RE.match(s, pos)
        if not m:
            return toks, s[pos:].strip() == ""
        pos = m.end()
        num, ident, op = m.groups()
        toks.append(("num", parse_number(num)) if num is not None else ("name", ident) if ident is not None
                    else ("**" if op == "^" else op,))
    return toks, True


class _Parser:
    """Precedence climbing over the token list; `expr(level)` reads operators that bind at least as tightly as `level`."""

    def __init__(self, toks):
        self.toks, self.i = toks, 0

    def peek(self):
        return self.toks[self.i][0] if self.i < len(self.toks) else None

    def take(self, want=None):
        tok = self.toks[self.i] if self.i < len(self.toks) else (None,)
        if want is not None and tok[0] != want:
            raise _Syntax("expected '%s' at token %d" % (want, self.i + 1))
        self.i += 1
        return tok

    def expr(self, level=0):
        left = self.operand(level)
        while _LBP.get(self.peek(), -1) >= level:
            op = self.take()[0]
            if op == "?":
                a = self.expr(_TERNARY)
                self.take(":")
                left = ("?", left, a, self.expr(_TERNARY))
            elif op == "**":
                left = (op, left, self.expr(_SIGN))
            elif op in ("&&", "||"):
                left = ("and" if op == "&&" else "or", left, self.expr(_LBP[op] + 1))
            else:
                left = (op, left, self.expr(_LBP[op] + 1))
                if _LBP[op] == _CMP and _LBP.get(self.peek()) == _CMP:
                    raise _Syntax("comparisons do not chain: parenthesise one of them")
        return left

    def operand(self, level):
        tok = self.take()
        kind = tok[0]
        if kind == "num":
            return tok
        if kind == "name":
            if self.peek() != "(":
                return tok
            self.take()
            args = []
            while self.peek() != ")":
                args.append(self.expr())
                if self.peek() != ")":
                    self.take(",")
            self.take()
            return ("call", tok[1], tuple(args))
        if kind == "(":
            inner = self.expr()
            self.take(")")
            return inner
        if kind in ("+", "-"):
            return ("neg" if kind == "-" else "pos", self.expr(_SIGN))
        if kind == "!" and level <= _NOT:
            return ("not", self.expr(_NOT))
        raise _Syntax("unexpected %s at token %d" % ("end" if kind is None else "'%s'" % kind, self.i))


def parse(toks):
    """Token list → tree; raises `CedarError` where the tokens are no expression."""
    p = _Parser(toks)
    try:
        tree = p.expr()
        if p.peek() is not None:
            raise _Syntax("unexpected '%s' at token %d" % (p.peek(), p.i + 1))
    except _Syntax as e:
        raise CedarError("invalid syntax: %s" % e)
    except RecursionError:
        raise CedarError("invalid syntax: nested too deeply")
    return tree


def evaluate(tree, env):
    """Value of `tree` with the identifiers of `env` (lower-case keys) shadowing `_FUNCS`.  Python arithmetic: the result can be
    a bool or a complex number, and the errors are Python's (`eval_expr` turns both into what a deck expects)."""
    tag = tree[0]
    if tag == "num":
        return tree[1]
    if tag == "name":
        return float(env[tree[1]]) if tree[1] in env else _FUNCS[tree[1]]
    if tag in _BINARY:
        return _BINARY[tag](evaluate(tree[1], env), evaluate(tree[2], env))
    if tag == "call":
        if tree[1] in env:
            raise TypeError("parameter '%s' is not a function" % tree[1])
        return _FUNCS[tree[1]](*[evaluate(a, env) for a in tree[2]])
    if tag == "neg":
        return -evaluate(tree[1], env)
    if tag == "pos":
        return +evaluate(tree[1], env)
    if tag == "not":
        return not evaluate(tree[1], env)
    if tag == "?":
        return evaluate(tree[2] if evaluate(tree[1], env) else tree[3], env)
    left = evaluate(tree[1], env)   # "and" / "or": the deciding operand, as in Python
    return evaluate(tree[2], env) if bool(left) == (tag == "and") else left


@functools.lru_cache(maxsize=4096)
def _compile(s):
    """Unquoted lower-case text → (identifiers in source order, tree or None, fault or None), memoised.  Nothing is raised here:
    a deck may hold a bad expression in a branch it never takes, so `eval_expr` reports the fault when the value is asked for —
    after the undefined identifiers that stand before a character no token starts with."""
    toks, whole = tokenize(s)
    names = tuple(t[1] for t in toks if t[0] == "name")
    if not whole:
        return names, None, "cannot parse expression %r"
    try:
        return names, parse(toks), None
    except CedarError as e:
        return names, None, "error evaluating %%r: %s" % e


def eval_expr(text, env):
    """Evaluate a SPICE expression against parameter environment `env` (dict, lowercase keys)."""
    s = text.strip().lower()
    if len(s) >= 2 and s[0] in "'{" and s[-1] in "'}":
        s = s[1:-1]
    v = parse_number(s)
    if v is not None:
        return v
    names, tree, fault = _compile(s)
    for n in names:
        if n not in env and n not in _FUNCS:
            raise CedarError("undefined parameter '%s' in expression %r" % (n, text))
    if fault is not None:
        raise CedarError(fault % text)
    try:
        return float(evaluate(tree, env))
    except Exception as e:  # noqa: BLE001
        raise CedarError("error evaluating %r: %s" % (text, e))
