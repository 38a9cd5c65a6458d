"""The SPICE front end (netlist.py, spice_expr.py) against tests/golden/netlist_trace.json, which make_netlist_trace.py recorded
from the commit before the front end was rewritten, with the few entries that the rewrite changes on purpose written by hand
there.  The corpus is tests/netlist_cases.py.  CPU only."""
import ast
import json
import os
import warnings

import pytest

import netlist_cases as nc
from cedarsim_jl_amd import netlist, spice_expr
from cedarsim_jl_amd.circuit import CedarError
from cedarsim_jl_amd.netlist import parse_spice

TRACE = json.load(open(os.path.join(nc.GOLD, "netlist_trace.json")))


def test_hand_written_expressions_reproduce_the_trace():
    assert [row[0] for row in TRACE["hand"]] == [text for text, _ in nc.HAND_EXPRESSIONS]
    for (text, env), (_, want) in zip(nc.HAND_EXPRESSIONS, TRACE["hand"]):
        assert nc.expression_trace(text, env) == want, (text, env)


def test_random_expressions_reproduce_the_trace():
    assert len(TRACE["random"]) == nc.N_RANDOM == 2000
    for seed, want in enumerate(TRACE["random"]):
        assert nc.expression_trace(nc.random_expression(seed), nc.RANDOM_ENV) == want, (seed, nc.random_expression(seed))


def test_error_messages_keep_their_prefixes():
    for text, prefix in (("a $ 1", "cannot parse expression 'a $ 1'"), ("foo+1", "undefined parameter 'foo' in expression 'foo+1'"),
                         ("c ? foo : 1", "undefined parameter 'foo' in expression"), ("foo $ 1", "undefined parameter 'foo'"),
                         ("1 $ foo", "cannot parse expression"), ("1/c", "error evaluating '1/c':"), ("a +", "error evaluating 'a +':"),
                         ("a<b<1", "error evaluating"), ("a//b", "error evaluating"), ("(-8)^0.5", "error evaluating")):
        with pytest.raises(CedarError) as e:
            spice_expr.eval_expr(text, nc.E)
        assert str(e.value).startswith(prefix), (text, str(e.value))


@pytest.mark.parametrize("name", list(nc.DECKS))
def test_deck_reproduces_the_trace(name):
    assert set(TRACE["decks"]) == set(nc.DECKS)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")   # "Statement ignored": the text is in the `warnings` group
        got = nc.deck_trace(*nc.DECKS[name])
    assert got == TRACE["decks"][name]


def test_taken_if_skips_every_later_branch_of_its_level():
    c = parse_spice(nc.IF_CHAIN).build()
    assert c.dev_names == ["r1", "v1"]
    assert parse_spice(nc.IF_CHAIN).build(s=2).dev_names == ["r2", "v1"] and parse_spice(nc.IF_CHAIN).build(s=3).dev_names == ["r3", "v1"]
    nl = parse_spice("* t\n.param s=1\n.if (s==1)\nr1 a 0 1\n.elseif (1/(s-1) > 0)\nr2 a 0 2\n.else\nr3 a 0 3\n.endif\n")
    assert nl.build().dev_names == ["r1"]        # the condition behind the taken branch is not evaluated
    assert nl.build(s=1.5).dev_names == ["r2"]
    with pytest.raises(CedarError):
        parse_spice("* t\n.param s=1\n.if (s==2)\nr1 a 0 1\n.elseif (1/(s-1) > 0)\nr2 a 0 2\n.endif\n").build()


def _plain(x):
    """A deep copy with every object (ParsedNetlist, Subckt) replaced by its class name and attributes."""
    if isinstance(x, dict):
        return {k: _plain(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return type(x).__name__, [_plain(v) for v in x]
    return (type(x).__name__, _plain(vars(x))) if hasattr(x, "__dict__") else x


def _snapshot(nl):
    return _plain({k: v for k, v in vars(nl).items() if k != "warnings"})


@pytest.mark.parametrize("name", ["hierarchy", "mos", "directives", "if_nested", "va_modules"])
def test_build_writes_nothing_onto_the_netlist(name):
    parse, overrides = nc.DECKS[name]
    nl = parse()
    before, keys = _snapshot(nl), set(vars(nl))
    assert keys == {"title", "top", "subckts", "models", "options", "tran", "warnings"}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for ov in overrides:
            try:
                nl.build(**ov)
            except CedarError:
                pass
            assert set(vars(nl)) == keys
            assert _snapshot(nl) == before


def test_alternating_builds_of_one_netlist_equal_builds_run_alone():
    for name, (parse, overrides) in nc.DECKS.items():
        good = [ov for ov, row in zip(overrides, TRACE["decks"][name]) if isinstance(row, dict)]
        if name in ("directives",) or len(good) < 2:   # `directives` appends to nl.warnings with every build
            continue
        alone = [nc.circuit_groups(nl, nl.build(**ov)) for ov in good for nl in [parse()]]
        shared = parse()
        for _ in range(2):
            for ov, want in zip(good, alone):
                assert nc._canon(nc.circuit_groups(shared, shared.build(**ov))) == nc._canon(want), (name, ov)


def test_front_end_calls_no_eval_exec_or_compile():
    for mod in (netlist, spice_expr):
        tree = ast.parse(open(mod.__file__).read())
        calls = [n.func for n in ast.walk(tree) if isinstance(n, ast.Call)]
        assert not {f.id for f in calls if isinstance(f, ast.Name)} & {"eval", "exec", "compile"}, mod.__name__
        # as an attribute, `compile` is allowed on the `re` module alone
        attrs = {(f.value.id if isinstance(f.value, ast.Name) else "?", f.attr) for f in calls if isinstance(f, ast.Attribute)}
        assert not {a for a in attrs if a[1] in ("eval", "exec", "compile")} - {("re", "compile")}, mod.__name__
        assert not {n.id for n in ast.walk(tree) if isinstance(n, ast.Name)} & {"eval", "exec", "builtins", "__builtins__"}, mod.__name__
