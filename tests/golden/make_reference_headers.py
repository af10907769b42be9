#!/usr/bin/env python3
"""Regenerate tests/golden/reference_headers.json from a checkout of the reference project.

    python tests/golden/make_reference_headers.py <reference checkout>

The fixture is data parsed out of the reference's barlib headers and HMC.cc (member names and types, function-pointer
names, four signatures, the call order in HamiltonianMC) by tests/test_reference_headers.py::parse_reference; no text of
the reference is stored.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests.test_reference_headers import FIXTURE, parse_reference  # noqa: E402


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    d = parse_reference(os.path.join(sys.argv[1], "barlib"))
    with open(FIXTURE, "w") as f:
        json.dump(d, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", os.path.relpath(FIXTURE))


if __name__ == "__main__":
    main()
