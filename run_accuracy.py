#!/usr/bin/env python3
"""Repo-root launcher of the accuracy harness: `python run_accuracy.py -m DIR --tokens-file ids.npy --prefill-policy 0 ...`."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "isca-2025-lia_amd"))
from lia_amd.run_accuracy import main  # noqa: E402

if __name__ == "__main__":
    main(sys.argv[1:])
