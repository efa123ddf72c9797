"""Fixture generator for tests/test_reference_registry.py (needs a checkout of the reference GraphGym).

    python tests/golden/make_register_golden.py <reference checkout>

Records what the reference's graphgym/register.py raises when a key is registered twice, for the keys the test
probes, as tests/golden/reference_register.json:

    duplicate_key_error   {key: str(KeyError) raised by register(key, ..., {key: ...})}

This is data (the messages the reference produces), not reference source.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
KEYS = ["x", "gcnidconv"]


def main(ref):
    sys.path.insert(0, ref)
    import graphgym.register as reg
    out = {}
    for k in KEYS:
        try:
            reg.register(k, 1, {k: 0})
        except KeyError as e:
            out[k] = str(e)
        else:
            sys.exit(f"register() accepted a duplicate of {k!r}")
    path = os.path.join(HERE, "reference_register.json")
    with open(path, "w") as f:
        json.dump({"duplicate_key_error": out}, f, indent=1)
        f.write("\n")
    print(path)


if __name__ == "__main__":
    if len(sys.argv) != 2 or not os.path.isdir(os.path.join(sys.argv[1], "graphgym")):
        sys.exit("usage: make_register_golden.py <reference checkout containing graphgym/>")
    main(sys.argv[1])
