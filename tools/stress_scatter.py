#!/usr/bin/env python3
"""Randomised GPU stress of the triangle scatter: the command line of tests/stress_scatter.py (--cases --seed --batch --first --oracle)."""
import os, runpy
runpy.run_path(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "stress_scatter.py"), run_name="__main__")
