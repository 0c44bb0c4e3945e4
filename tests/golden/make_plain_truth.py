#!/usr/bin/env python3
"""Generates tests/golden/plain_truth_v1.json: the reference's own plaintext truth functions (test/plain.h, namespace
cufhe, NandCheck ... NMuxCheck) evaluated on every input combination, read through oracle/_ref/libplain_ref.so.

The fixture lets tests/test_oracle.py pin the oracle's truth tables to the reference's on a machine where
oracle/_ref was never built; where it was, the same test checks the library against the fixture.
    make -C oracle ref && python tests/golden/make_plain_truth.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import oracle_lib as ol  # noqa: E402

COMBOS = [(a, b, c) for a in (0, 1) for b in (0, 1) for c in (0, 1)]


def main():
    if ol.ref_plain() is None:
        sys.exit("oracle/_ref/libplain_ref.so is missing: build it with `make -C oracle ref` where the reference tree is mounted")
    fx = {"version": 1, "source": "test/plain.h of the reference through oracle/_ref/libplain_ref.so",
          "inputs": [list(c) for c in COMBOS],
          "gates": {name: [ol.ref_truth(name, *c) for c in COMBOS] for name in ol.REF_NAMES}}
    with open(os.path.join(HERE, "plain_truth_v1.json"), "w") as f:
        json.dump(fx, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
