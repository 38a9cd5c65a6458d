"""Writes tests/golden/netlist_trace.json: what the SPICE front end does with the corpus of tests/netlist_cases.py.

  "hand":   [text, `float.hex()` of the value or "CedarError"] for every entry of HAND_EXPRESSIONS, in its order;
  "random": the same for random_expression(seed), seeds 0..1999 (RANDOM_ENV);
  "decks":  per deck, one entry per override set: a 16-hex sha256 digest per field group (nodes, devices, sources, models,
            va_par, spec, tran_options, warnings), or the class name of what `build` raised.

Recorded from the commit BEFORE netlist.py was split (expressions went through a translation to Python source and `eval`), so that
the test compares the rewritten front end with its parent and not with itself.  At that commit 1524 of the 2000 random expressions
(76.2 %) evaluate to a finite number, the rest are error paths or infinities.  Run it again only when the front end is changed on purpose.

What the rewrite changes on purpose is not taken from that commit but written here by hand: see `by_hand` below."""
import json
import math
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
import netlist_cases as nc  # noqa: E402


def by_hand(hand, decks):
    # Nested and parenthesised ternaries were syntax errors (the ternary was a textual split on the first `?`); they evaluate now.
    want = {text: float(value).hex() for text, value in nc.NESTED_TERNARIES}
    # Two accidents of the translation to Python are errors now: `a<b<1` chained as in Python, `a//b` was floor division.
    want.update({text: "CedarError" for text in nc.REJECTED_ACCIDENTS})
    for row in hand:
        row[1] = want.get(row[0], row[1])
    # `.if (s==1) r1 .elseif (s==2) r2 .else r3 .endif` with s=1 built r1 AND r3: `.elseif` and `.else` looked at the branch just
    # before them only, so after a taken branch every second one could be taken again.  Expected is the circuit of the same deck
    # written without the conditional (same title, parameters and element order): netlist_cases.CORRECTED.
    for (deck, i), corrected in nc.CORRECTED.items():
        decks[deck][i] = nc.deck_trace(corrected, [nc.DECKS[deck][1][i]])[0]


if __name__ == "__main__":
    hand = [[text, nc.expression_trace(text, env)] for text, env in nc.HAND_EXPRESSIONS]
    rnd = [nc.expression_trace(nc.random_expression(s), nc.RANDOM_ENV) for s in range(nc.N_RANDOM)]
    finite = sum(r != "CedarError" and math.isfinite(float.fromhex(r)) for r in rnd)
    print("random expressions with a finite value: %d of %d (%.1f %%)" % (finite, len(rnd), 100.0 * finite / len(rnd)))
    assert finite >= 0.6 * len(rnd)
    decks = {name: nc.deck_trace(parse, ovs) for name, (parse, ovs) in nc.DECKS.items()}
    by_hand(hand, decks)
    with open(os.path.join(HERE, "netlist_trace.json"), "w") as f:
        f.write('{"hand": [\n' + ",\n".join(json.dumps(hand[i:i + 4])[1:-1] for i in range(0, len(hand), 4)) + '\n],\n"random": [\n')
        f.write(",\n".join(json.dumps(rnd[i:i + 8])[1:-1] for i in range(0, len(rnd), 8)) + '\n],\n"decks": {\n')
        f.write(",\n".join("%s: %s" % (json.dumps(k), json.dumps(v)) for k, v in decks.items()) + "\n}}\n")
