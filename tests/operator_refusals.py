"""What tests/test_operator_refusals.py and tests/test_gpu_operator_refusals.py share: the records of
``golden/operator_refusals.json`` and how a refused call becomes one.

A record is ``{"call", "args", "rc", "message"}``: the C function, its arguments as written in the case lists, the return
code and the bytes of ``saa_last_error()`` after the call.  An argument is written as a number, ``None`` (a null pointer),
a string (an option name, passed as bytes; ``"nan"``, ``"inf"`` and ``"-inf"`` are the floats) or ``"@name"``, which is
looked up in the environment the test built (handles, buffers, sizes of its mesh).  The fixture was recorded from the
library before the guards of the operator family were gathered into helpers; the comparison is exact, so that neither a
code, nor a byte of a message, nor the order of two checks of one function moves."""
import json
import os

from conftest import GOLDEN

FIXTURE = os.path.join(GOLDEN, "operator_refusals.json")
FLOATS = {"nan": float("nan"), "inf": float("inf"), "-inf": float("-inf")}


def resolve(arg, env):
    if not isinstance(arg, str):
        return arg
    if arg.startswith("@"):
        return env[arg[1:]]
    return FLOATS[arg] if arg in FLOATS else arg.encode()


def call(lib, name, args, env):
    """The record of one call."""
    rc = getattr(lib, name)(*[resolve(a, env) for a in args])
    return {"call": name, "args": list(args), "rc": int(rc), "message": (lib.saa_last_error() or b"").decode()}


def keys(cases):
    """One key per ``(call, args)`` of ``cases``, in order: the call, its arguments and how often the pair came before (the
    same call is refused for another reason once the state of its handle has changed)."""
    seen, out = {}, []
    for name, args in cases:
        k = (name, json.dumps(list(args)))
        out.append(k + (seen.get(k, 0),))
        seen[k] = seen.get(k, 0) + 1
    return out


def _fixture():
    if not os.path.exists(FIXTURE):
        return [], []
    with open(FIXTURE) as fh:
        records = json.load(fh)
    return records, keys([(r["call"], r["args"]) for r in records])


def expected(cases):
    """The fixture's records of ``cases``, in their order.  Every case must be there."""
    by_key = dict(zip(*reversed(_fixture())))
    return [by_key[k] for k in keys(cases)]


def compare(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert w["rc"] != 0, w                                              # a refusal, or the message is the previous call's
        assert g == w, f"{g['call']}{tuple(g['args'])}: {g['rc']} {g['message']!r}, expected {w['rc']} {w['message']!r}"


def write(records, first):
    """Replaces this part's records in the fixture and keeps the other part's: ``first`` puts them in front."""
    mine = set(keys([(r["call"], r["args"]) for r in records]))
    assert all(r["rc"] != 0 for r in records), [r for r in records if r["rc"] == 0]
    others = [r for r, k in zip(*_fixture()) if k not in mine]
    with open(FIXTURE, "w") as fh:
        fh.write("[\n" + ",\n".join(json.dumps(r) for r in (records + others if first else others + records)) + "\n]\n")
    pairs = {(r["call"], r["message"]) for r in records}
    print(f"wrote {FIXTURE}: {len(records)} records of this part ({len(pairs)} distinct (function, message) pairs), "
          f"{len(others)} kept, {os.path.getsize(FIXTURE)} bytes")
