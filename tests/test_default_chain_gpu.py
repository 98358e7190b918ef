"""The DEFAULT chain -- ``DeviceDeform`` / ``FusionScanPipeline`` with the class-aware fusion (``LT_TSDF_MERGE``) -- against an
independent chain made of reference code (tests/oracle_chain.py: the reference's own ``integrate`` kernel source, marching
cubes = scikit-image's arrays, the reference raytracer, numpy restatements of the projection, the mergemesh bounds and
``write()``).  Every output scan: volumes bit-identical, the renumbered mesh element for element, the images under the
equality rule of ``oracle_chain.check_images`` (bit for bit but for exact-t ties, at most 1e-3 of the rays), the written bytes
equal.  Configurations: the 16 seeded F13b / F14b sensor models, a 64 x 2048 source (above 81 920 pixels the integrate kernels'
workgroups walk several pixel groups), the four F14c sequences one scan at a time (one native call, and composed from the
public steps) and in flight (3 and 4 chains), the benchmark's timed outputs, and a sequence in flight that loses a scan."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if HERE not in sys.path:
    sys.path.insert(0, HERE)

BIG_SOURCE = (64, 2048, 3.0, -25.0)
BIG_TARGET = (32, 1024, 10.0, -30.0)
BIG_BNDS = np.array([[-12, 12], [-12, 12], [-3, 3]])
BIG_VOXEL, BIG_SEED, BIG_SCANS = 0.1, 4242, 3
TIE_BOUND = 1e-3


def _need_reference_builds():
    from oracle import binding as ob
    if not ob.ref_available("strict"):
        pytest.skip("oracle/_ref/libref_strict.so not built (needs /root/reference at build time)")
    if not ob.ref_tsdf_available():
        pytest.skip("oracle/_ref/libref_tsdf_integrate.so not built (needs /root/reference + hipcc at build time)")


def _host_render(v, f, c, r, H, W, fu, fd):
    """source clouds: the hit points of the reference's search (restated, the goldens' RSQRTSS seed) -- no product code"""
    import oracle_chain as oc
    from oracle import binding as ob
    o = ob.oracle_trace(oc.create_rays(fu, fd, H, W), np.zeros(3, np.float32), v, f, c, r, H, mode=ob.MODE_REF_BVH,
                        norm=ob.NORM_SSE_TABLE, nthreads=oc.THREADS)
    return o["endpoints"], o["endcolors"][:, 2], o["endrem"], o["range"]


def _dev(clouds):
    import torch
    return [(torch.from_numpy(p).cuda(), torch.from_numpy(r).cuda(), torch.from_numpy(l.astype(np.int32)).cuda())
            for p, r, l in clouds]


def _mesh_cases():
    """(name, source, target, vol_bnds, voxel, clouds) of every DeviceDeform.mesh case: the 16 seeded configurations (each one
    output scan, its first seed) and the 64 x 2048 one"""
    import pin_cases
    out = []
    for k in range(pin_cases.N_DEFORM_MESH_CASES):
        _, src, tgt, n_scans, bnds, voxel, seeds = pin_cases.deform_mesh_case(k)
        out.append((f"c{k}", src, tgt, bnds, voxel, pin_cases.deform_mesh_clouds(seeds[0], n_scans, src, _host_render)))
    out.append(("big", BIG_SOURCE, BIG_TARGET, BIG_BNDS, BIG_VOXEL,
                pin_cases.deform_mesh_clouds(BIG_SEED, BIG_SCANS, BIG_SOURCE, _host_render)))
    return out


_ORACLE = {}


def _oracle_mesh(case):
    import oracle_chain as oc
    name, src, tgt, bnds, voxel, clouds = case
    if name not in _ORACLE:
        want = oc.deform_mesh(clouds, src, tgt, bnds, voxel)
        want["fields"] = [t.cpu() for t in want.pop("volume").fields]
        _ORACLE[name] = want
    return _ORACLE[name]


def _seq_inputs(k):
    import pin_cases
    src, tgt, bnds, voxel, seed, limits = pin_cases.mergemesh_seq_case(k)
    return src, tgt, bnds, voxel, [pin_cases.mergemesh_seq_clouds(seed, src, _host_render, lim) for lim in limits]


def _oracle_seq(k, drop=()):
    """the oracle chain over sequence k (scans in ``drop`` never happened: their bounds statements did not run)"""
    import oracle_chain as oc
    key = ("seq", k, tuple(drop))
    if key not in _ORACLE:
        src, tgt, bnds, voxel, clouds = _seq_inputs(k)
        b = bnds.copy()
        outs = []
        for step, c in enumerate(clouds):
            if step in drop:
                outs.append(None)
                continue
            w = oc.deform_mergemesh(c, src, tgt, b, voxel)
            w["fields"] = [t.cpu() for t in w.pop("volume").fields]
            outs.append(w)
        _ORACLE[key] = outs
    return _ORACLE[key]


def _check_volumes(tensors, want, tag):
    import torch
    for name, a, b in zip(("tsdf", "weight", "color", "rem"), tensors, want["fields"]):
        a = a.cpu().contiguous()
        assert tuple(a.shape) == tuple(b.shape), f"{tag}: {name} shape {tuple(a.shape)} vs {tuple(b.shape)}"
        bad = int((a.view(torch.int32) != b.contiguous().view(torch.int32)).sum())
        assert bad == 0, f"{tag}: {bad} voxels of {name} differ from the reference kernel's"


def _check_mesh(mesh_obj, want, tag):
    v, f, c, r = [t.cpu().numpy() for t in mesh_obj.renumber().tensors()]
    wv, wf, wc, wr = want["mesh"]
    assert v.shape == wv.shape and f.shape == wf.shape, f"{tag}: mesh sizes {v.shape} {f.shape} vs {wv.shape} {wf.shape}"
    assert np.array_equal(v.view(np.int32), wv.view(np.int32)), f"{tag}: vertices"
    assert np.array_equal(f, wf), f"{tag}: faces"
    assert np.array_equal(c.astype(np.int64), wc.astype(np.int64)), f"{tag}: vertex colours"
    assert np.array_equal(r.view(np.int32), wr.view(np.int32)), f"{tag}: vertex remissions"


def _images(got, label_key="label", rem_key="rem"):
    return dict(range=got["range"].cpu().numpy(), label=got[label_key].cpu().numpy(), rem=got[rem_key].cpu().numpy(),
                endpoints=got["endpoints"].cpu().numpy(), tri=got["tri"].cpu().numpy())


def _check_scan(got, want, tag, ties):
    import oracle_chain as oc
    n = oc.check_images(_images(got), want, tag)
    assert n[0] <= TIE_BOUND * want["ref"]["range"].size, f"{tag}: {n[0]} exact-t tie pixels"
    ties[tag] = n
    if n == (0, 0):
        assert np.array_equal(want["bin_rule"].view(np.uint8), want["bin"].view(np.uint8))
    assert np.array_equal(got["bin"].cpu().numpy().view(np.uint8), want["bin_rule"].view(np.uint8)), f"{tag}: velodyne bytes"
    assert np.array_equal(got["label_file"].cpu().numpy().view(np.uint32), want["label_file_rule"]), f"{tag}: label bytes"


def test_default_mesh_adaption_equals_the_oracle_chain():
    """(a) DeviceDeform.mesh with the default fusion, the 16 seeded configurations and a 64 x 2048 source with three scans"""
    import torch
    from lidar_transfer_amd.deform import DeviceDeform
    _need_reference_builds()
    ties = {}
    for case in _mesh_cases():
        name, src, tgt, bnds, voxel, clouds = case
        want = _oracle_mesh(case)
        dd = DeviceDeform(src, tgt, bnds.copy(), voxel)
        assert dd._fusion == "cuda" and dd._merge_flag
        got = dd.mesh(_dev(clouds))
        torch.cuda.synchronize()
        assert tuple(int(x) for x in dd.vol._vol_dim) == want["vol_dim"], name
        _check_volumes(dd.vol.get_volume_tensors(), want, name)
        _check_scan(got, want, name, ties)
        _check_mesh(dd.mesh_obj, want, name)
        assert (want["ref"]["range"] > 0).sum() > 100, f"{name}: the oracle's image is nearly empty"
        dd.close()
    assert BIG_SOURCE[0] * BIG_SOURCE[1] > 81920
    print(f"\ndefault mesh chain vs the oracle chain: (exact-t tie pixels, in-plane pixels) per case {ties}")


@pytest.mark.parametrize("source_images", [False, True])
def test_default_mergemesh_sequences_equal_the_oracle_chain(source_images):
    """(b) DeviceDeform.mergemesh with the default fusion: the four F14c sequences, six scans each on ONE bounds array, through
    the one-call path and composed from the public steps (whose merged-cloud images are compared with the oracle's projection)"""
    import torch
    from lidar_transfer_amd.deform import DeviceDeform
    _need_reference_builds()
    ties, reruns = {}, 0
    for k in range(4):
        src, tgt, bnds, voxel, clouds = _seq_inputs(k)
        want = _oracle_seq(k)
        b = bnds.copy()
        dd = DeviceDeform(src, tgt, b, voxel, mesh_volume=False)
        for step, c in enumerate(clouds):
            tag = f"q{k}s{step}"
            w = want[step]
            got = dd.mergemesh(_dev(c), source_images=source_images)
            torch.cuda.synchronize()
            assert got["vol_dim"] == w["vol_dim"], (tag, got["vol_dim"], w["vol_dim"])
            assert np.array_equal(b, w["bnds_after"]) and b.dtype == w["bnds_after"].dtype, (tag, b, w["bnds_after"])
            assert np.array_equal(np.asarray(got["vol_origin"], np.float32).view(np.int32), w["vol_origin"].view(np.int32)), tag
            _check_volumes(got["volume"].get_volume_tensors(), w, tag)
            _check_scan(got, w, tag, ties)
            _check_mesh(dd.mesh_obj, w, tag)
            if source_images:
                s = got["source"]
                assert np.array_equal(s["range"].cpu().numpy().view(np.int32), w["source"]["range"].view(np.int32)), tag
                assert np.array_equal(s["rem"].cpu().numpy().view(np.int32), w["source"]["rem"].view(np.int32)), tag
                folded = (w["source"]["label"].astype(np.float32) * np.float32(65536)).astype(np.float32)
                assert np.array_equal(s["label_folded"].cpu().numpy().astype(np.float32), folded), tag
        reruns += dd._mm_state.stats["rerun"]
        dd.close()
    assert reruns >= 8
    print(f"\ndefault mergemesh chain (source_images={source_images}) vs the oracle chain: (exact-t tie pixels, in-plane pixels) {ties}")


def _check_pipeline_scan(got, w, tag, ties):
    import oracle_chain as oc
    n = oc.check_images(dict(range=got["range"].cpu().numpy(), label=got["endcolors"].cpu().numpy(),
                             rem=got["endrem"].cpu().numpy(), endpoints=got["endpoints"].cpu().numpy(),
                             tri=got["tri"].cpu().numpy()), w, tag)
    assert n[0] <= TIE_BOUND * w["ref"]["range"].size, f"{tag}: {n[0]} exact-t tie pixels"
    ties[tag] = n


@pytest.mark.parametrize("chains", [3, 4])
def test_mergemesh_in_flight_equals_the_oracle_chain(chains):
    """(c) FusionScanPipeline.submit_mergemesh: the four sequences with 3 / 4 scans in flight, every scan against the ORACLE
    chain; the bounds move inside every sequence, so scans launched on the previous geometry are run again"""
    from lidar_transfer_amd.laserscan import create_rays_device
    from lidar_transfer_amd.pipeline import FusionScanPipeline
    _need_reference_builds()
    ties, reruns = {}, 0
    for k in range(4):
        src, tgt, bnds, voxel, clouds = _seq_inputs(k)
        want = _oracle_seq(k)
        b = bnds.copy()
        rays = create_rays_device(tgt[2], tgt[3], tgt[0], tgt[1], device=0)
        with FusionScanPipeline(b, voxel, tgt[2], tgt[3], rays, tgt[0], chains=chains, device=0, label_image=True,
                                source_hw=(src[0], src[1]), fixed_volume=False) as pipe:
            tickets = [pipe.submit_mergemesh(_dev(c), inputs_ready=True) for c in clouds]
            for step, t in enumerate(tickets):
                got = pipe.wait(t)
                w = want[step]
                tag = f"q{k}s{step}/{chains}"
                assert tuple(got["vol_dim"]) == w["vol_dim"], tag
                assert np.array_equal(np.array(got["vol_bnds_after"]).reshape(3, 2), w["bnds_after"].astype(np.float64)), tag
                _check_pipeline_scan(got, w, tag, ties)
            pipe.flush()
            assert np.array_equal(b, want[-1]["bnds_after"]) and b.dtype == want[-1]["bnds_after"].dtype
            reruns += pipe._mm_state.stats["rerun"]
    assert reruns >= 1, "no geometry change forced a rerun"
    print(f"\n{chains} mergemesh chains in flight vs the oracle chain: {reruns} reruns; (exact-t tie pixels, in-plane pixels) {ties}")


def test_clouds_in_flight_equal_the_oracle_chain():
    """(c) FusionScanPipeline.submit_clouds, 3 chains: every mesh case's output scan three times in flight"""
    import torch
    from lidar_transfer_amd.laserscan import create_rays_device
    from lidar_transfer_amd.pipeline import FusionScanPipeline
    _need_reference_builds()
    ties = {}
    for case in _mesh_cases():
        name, src, tgt, bnds, voxel, clouds = case
        want = _oracle_mesh(case)
        rays = create_rays_device(tgt[2], tgt[3], tgt[0], tgt[1], device=0)
        with FusionScanPipeline(bnds.copy(), voxel, src[2], src[3], rays, tgt[0], chains=3, device=0, label_image=True,
                                source_hw=(src[0], src[1])) as pipe:
            dev = _dev(clouds)
            tickets = [pipe.submit_clouds(dev, inputs_ready=True) for _ in range(3)]
            for j, t in enumerate(tickets):
                _check_pipeline_scan(pipe.wait(t), want, f"{name}/{j}", ties)
        torch.cuda.synchronize()
    print(f"\nsubmit_clouds, 3 chains in flight, vs the oracle chain: (exact-t tie pixels, in-plane pixels) {ties}")


_LOST_SCAN_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[2])
import torch
import test_default_chain_gpu as t
import oracle_chain as oc
from lidar_transfer_amd.laserscan import create_rays_device
from lidar_transfer_amd.pipeline import FusionScanPipeline
src, tgt, bnds, voxel, clouds = t._seq_inputs(0)
want = t._oracle_seq(0, drop=(2,))
b = bnds.copy()
rays = create_rays_device(tgt[2], tgt[3], tgt[0], tgt[1], device=0)
with FusionScanPipeline(b, voxel, tgt[2], tgt[3], rays, tgt[0], chains=3, device=0, label_image=True,
                        source_hw=(src[0], src[1]), fixed_volume=False) as pipe:
    try:
        pipe.submit_mergemesh([])
        raise SystemExit("an empty submission was accepted")
    except ValueError:
        pass
    scene = pipe._chains[2]["scene"]
    def fail(*a, **k):
        del scene.alloc_outputs                           # (once: chain 2's later jobs allocate as usual)
        raise MemoryError("injected: output allocation of scan 2")
    scene.alloc_outputs = fail                            # chain 2's first job is the sequence's scan 2
    tickets = [pipe.submit_mergemesh(t._dev(c), inputs_ready=True) for c in clouds]
    ties = {}
    for step, tk in enumerate(tickets):
        if step == 2:
            try:
                pipe.wait(tk)
                raise SystemExit("scan 2 did not fail")
            except MemoryError:
                continue
        got = pipe.wait(tk)
        w = want[step]
        assert tuple(got["vol_dim"]) == w["vol_dim"], step
        t._check_pipeline_scan(got, w, f"s{step}", ties)
    pipe.flush()
    assert np.array_equal(b, want[-1]["bnds_after"])
print("LOST_SCAN_OK", ties)
"""


def test_a_mergemesh_scan_that_fails_does_not_block_its_sequence():
    """an empty submit_mergemesh is refused before the sequence number moves, and a scan whose output allocation
    fails gives up its turn -- the later scans of the sequence complete and equal the oracle chain run without that scan.  In a
    child process under a time limit: a regression hangs the child (the later scans wait for a turn that never comes), not the
    suite."""
    _need_reference_builds()
    try:
        res = subprocess.run([sys.executable, "-c", _LOST_SCAN_CHILD, HERE, ROOT], capture_output=True, text=True, timeout=300,
                             cwd=ROOT)
    except subprocess.TimeoutExpired:
        pytest.fail("the sequence blocked after a failed scan (child process timed out)")
    assert res.returncode == 0 and "LOST_SCAN_OK" in res.stdout, (res.stdout[-2000:], res.stderr[-3000:])
    print("\n" + res.stdout.strip().splitlines()[-1])


def test_benchmark_timed_outputs_equal_the_reference_raytracer(tmp_path):
    """bench.py's last timed step (--dump-outputs: a seeded sample of 32 768 cells of the last 64 scans, end points / remissions
    / triangles of the held ones): every scan's range and label equal the reference raytracer's image of exactly one of the four
    scenes, the scans cycle through the scenes in order, the held scans follow the equality rule"""
    import oracle_chain as oc
    from lidar_transfer_amd.synth import WORKLOADS, synth_scene
    from tools import bench_lib
    _need_reference_builds()
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    d = tmp_path / "dump"
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                          "--workload", "C1", "--scenes", "4", "--dump-outputs", str(d)], capture_output=True, text=True,
                         timeout=900, env=env, cwd=ROOT)
    assert res.returncode == 0, res.stderr[-3000:]
    files = {p.stem: np.load(p) for p in sorted(d.glob("*.npy"))}
    wl = WORKLOADS["C1"]
    H, W = wl["H"], wl["W"]
    cells = np.sort(np.random.default_rng(bench_lib.DUMP_SEED).choice(H * W, size=min(H * W, bench_lib.DUMP_RAYS), replace=False))
    assert files["range"].shape == (bench_lib.DUMP_SCANS, len(cells))
    want = []
    for i in range(4):
        v, f, c, r = synth_scene(i, wl["tris"])
        ref, brute = oc.render((v, f, c, r), (H, W, wl["fov_up"], wl["fov_down"]))
        sub = lambda o: {k: np.asarray(o[k])[cells] for k in ("range", "endrem", "endpoints", "endcolors", "tri", "rays") if k in o}  # noqa
        want.append(dict(ref=sub(ref), brute=sub(brute)))

    def expected(w):      # (the rule of oracle_chain.check_images on range and label)
        ref, brute = w["ref"], w["brute"]
        rb, bb = ref["range"].view(np.int32), brute["range"].view(np.int32)
        differ = (rb != bb) | (ref["endcolors"][:, 2] != brute["endcolors"][:, 2]) | (ref["endrem"].view(np.int32) !=
                                                                                     brute["endrem"].view(np.int32))
        in_plane = (np.abs(ref["rays"]) < 1e-7).any(1)
        use_brute = differ & ((rb == bb) | in_plane)
        return np.where(use_brute, bb, rb), np.where(use_brute, brute["endcolors"][:, 2], ref["endcolors"][:, 2])

    exp = [expected(w) for w in want]
    scene_of = []
    for row in range(files["range"].shape[0]):
        rb, lab = files["range"][row].astype(np.float32).view(np.int32), files["label"][row].astype(np.int64)
        hits = [i for i, (er, el) in enumerate(exp) if np.array_equal(rb, er) and np.array_equal(lab, el)]
        assert len(hits) == 1, f"dumped scan {row}: equals the reference image of scenes {hits}"
        scene_of.append(hits[0])
    assert all((b - a) % 4 == 1 for a, b in zip(scene_of, scene_of[1:])), scene_of
    n_held = files["tri"].shape[0]
    assert n_held >= 1
    ties = {}
    for j in range(n_held):
        row = files["range"].shape[0] - n_held + j
        w = want[scene_of[row]]
        got = dict(range=files["range"][row].astype(np.float32), label=files["label"][row].astype(np.int64),
                   rem=files["endrem"][j].astype(np.float32), endpoints=files["endpoints"][j].astype(np.float32),
                   tri=files["tri"][j].astype(np.int64))
        n = oc.check_images(got, w, f"held scan {row}")
        assert n[0] <= TIE_BOUND * len(cells)
        ties[row] = n
    print(f"\nbench C1 timed outputs: {len(scene_of)} scans equal the reference raytracer (scenes {scene_of[:8]}...); "
          f"held scans' (exact-t tie pixels, in-plane pixels) {ties}")
