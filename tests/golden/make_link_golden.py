#!/usr/bin/env python3
"""The library symbols a translation unit built on the reference's own headers refers to (DATA: mangled names).

Run in the build container only, after build(): compiles tests/link_ref/link_ref_headers.cpp against the reference's
include directory and keeps the undefined symbols of the object that libcusk_hip.so defines.  Writes
ref_link_symbols.json, which tests/test_cli_and_abi.py compares with the symbols of tests/link_ref/link_ref_decls.cpp.

Usage: python tests/golden/make_link_golden.py <reference checkout>
"""
import json
import os
import subprocess
import sys
import tempfile

REF = sys.argv[1] if len(sys.argv) > 1 else sys.exit(__doc__)
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
from test_cli_and_abi import library_symbols, undefined_symbols  # noqa: E402


def main():
    with tempfile.TemporaryDirectory() as d:
        obj = os.path.join(d, "h.o")
        subprocess.run(["g++", "-std=c++20", "-I" + os.path.join(REF, "cusk", "include"), "-c",
                        os.path.join(ROOT, "tests", "link_ref", "link_ref_headers.cpp"), "-o", obj], check=True)
        syms = sorted(undefined_symbols(obj) & library_symbols())
    with open(os.path.join(HERE, "ref_link_symbols.json"), "w") as f:
        json.dump({"source": "tests/link_ref/link_ref_headers.cpp compiled against the reference's cusk/include",
                   "symbols": syms}, f, indent=1)
        f.write("\n")
    print(syms)


if __name__ == "__main__":
    main()
