"""Randomised comparisons with the two checkers that ARE the reference's code run here -- short versions of the stress runs of
tools/r04/r04_final.sh (tests/stress_mc.py 300 volumes, tests/stress_tsdf_ref.py 300 configurations; profiles/r04/gpu_suite.txt)
-- and a short version of the ray cast's random stress (tests/stress_scatter.py) against the LBVH strategy and the oracle."""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def test_marching_cubes_on_random_volumes_equals_scikit_images_arrays(oracle):
    import stress_mc
    assert stress_mc.main(["stress_mc", "60", "11"]) == 0


def test_integrate_on_random_configurations_equals_the_reference_kernel_build():
    from oracle import binding as ob
    if not ob.ref_tsdf_available():
        pytest.skip("oracle/_ref/libref_tsdf_integrate.so not built (needs /root/reference + hipcc at build time)")
    import stress_tsdf_ref
    assert stress_tsdf_ref.main(["stress_tsdf_ref", "60", "11"]) == 0


def test_scatter_on_random_cases_equals_lbvh_and_the_brute_force_oracle(oracle):
    """The random stress of the ray cast (tests/stress_scatter.py: grids beyond the bin grid's 4096 rows / 8192 columns,
    seamless, two-block and jittered grids, rays sharing a direction, low-poly scenes, far origins, broken meshes): the
    scatter render against the LBVH strategy, against the brute-force oracle where triangles x rays < 3e7 (26 of seed
    11's first 40 cases), and once more through the batch call in groups of up to 8."""
    import importlib.util  # by path: tools/stress_scatter.py, the command line, has the same module name
    spec = importlib.util.spec_from_file_location("tests_stress_scatter", os.path.join(os.path.dirname(os.path.abspath(__file__)), "stress_scatter.py"))
    stress_scatter = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(stress_scatter)
    summary = {}
    assert stress_scatter.main(["stress_scatter", "--cases", "40", "--seed", "11", "--oracle", "--batch", "8"], summary) == 0
    assert summary["cases"] == 40 and summary["n_batched"] == 40
    assert summary["n_oracle"] >= 24, summary
