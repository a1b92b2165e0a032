"""Multi-atlas segmentation harness (platipy_amd.projects.multiatlas.run_segmentation) on the reference's own
acceptance data -- synthetic spheres, Dice of the fused whole-heart contour (platipy/imaging/tests/test_cardiac.py:142
asserts > 0.99 at full size with its full settings; this half-size, short-schedule CPU run asserts > 0.93) -- and the
world_size-2 `gloo` run of the same job: one atlas chain per rank, ONE all_reduce for the fusion."""
import copy
import os

import numpy as np
import pytest
import torch

from tests.helpers import dice, sphere_case

ORIGIN = (320.0, -52.0, 60.0)


def _settings(ids):
    from platipy_amd.projects.multiatlas import MUTLIATLAS_SETTINGS_DEFAULTS

    s = copy.deepcopy(MUTLIATLAS_SETTINGS_DEFAULTS)
    s["atlas_settings"]["atlas_id_list"] = ids
    s["atlas_settings"]["atlas_structure_list"] = ["WHOLEHEART", "SUBSTRUCTURE"]
    s["auto_crop_target_image_settings"]["expansion_mm"] = [8, 8, 10]
    s["linear_registration_settings"].update({"shrink_factors": [4, 2], "smooth_sigmas": [0, 0], "number_of_iterations": 20,
                                              "reg_method": "similarity"})
    s["deformable_registration_settings"].update({"isotropic_resample": False, "resolution_staging": [4, 2, 1],
                                                  "iteration_staging": [8, 8, 8], "smoothing_sigmas": [0, 0, 0]})
    s["label_fusion_settings"]["vote_type"] = "local"
    return s


def _data(pa, ids):
    atlases = {}
    for k, cid in enumerate(ids):
        ct, m, sub, sp = sphere_case(k)
        atlases[cid] = {"CT Image": pa.image_from_array(ct, sp, ORIGIN), "WHOLEHEART": pa.image_from_array(m, sp, ORIGIN),
                        "SUBSTRUCTURE": pa.image_from_array(sub, sp, ORIGIN)}
    ct, m, sub, sp = sphere_case(4)
    return pa.image_from_array(ct, sp, ORIGIN), m, sub, atlases


def test_run_segmentation_sphere_fixture(host_api):
    pa = host_api
    ids = ["001", "002", "003"]
    target, tmask, tsub, atlases = _data(pa, ids)
    streams = 2 if target.device.type == "cuda" else 1
    results, prob = pa.projects.multiatlas.run_segmentation(target, _settings(ids), atlases=atlases, streams_per_gpu=streams)
    assert set(results) == {"WHOLEHEART", "SUBSTRUCTURE"}
    wh = results["WHOLEHEART"]
    assert wh.GetSize() == target.GetSize() and wh.tensor.dtype == torch.uint8
    assert prob["WHOLEHEART"].GetSize() == target.GetSize()
    d = dice(wh.numpy(), tmask)
    assert d > 0.93, d
    assert dice(results["SUBSTRUCTURE"].numpy(), tsub) > 0.5
    p = prob["WHOLEHEART"].numpy()
    assert 0.0 <= p.min() and p.max() <= 1.0


def test_run_segmentation_reads_nifti_atlases(host_api, tmp_path):
    """Atlases on disk in the reference's layout (multiatlas/run.py:56-58) give the same result as in memory."""
    pa = host_api
    from platipy_amd.io import write_image

    ids = ["001", "002"]
    target, tmask, _, atlases = _data(pa, ids)
    st = _settings(ids)
    st["atlas_settings"]["atlas_path"] = str(tmp_path)
    for cid in ids:
        (tmp_path / f"Case_{cid}" / "Images").mkdir(parents=True)
        (tmp_path / f"Case_{cid}" / "Structures").mkdir(parents=True)
        write_image(atlases[cid]["CT Image"], tmp_path / st["atlas_settings"]["atlas_image_format"].format(cid))
        for s in ("WHOLEHEART", "SUBSTRUCTURE"):
            write_image(atlases[cid][s], tmp_path / st["atlas_settings"]["atlas_label_format"].format(cid, s))
    from_disk, _ = pa.projects.multiatlas.run_segmentation(target, st)
    in_mem, _ = pa.projects.multiatlas.run_segmentation(target, st, atlases=atlases)
    # float32 spacing in the NIfTI header perturbs the geometry by ~1e-8 relative: masks agree almost everywhere
    assert (from_disk["WHOLEHEART"].numpy() != in_mem["WHOLEHEART"].numpy()).mean() < 1e-3
    assert dice(from_disk["WHOLEHEART"].numpy(), tmask) > 0.9


def _worker(rank, world, port, out_dir):
    os.environ.update({"MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port), "RANK": str(rank), "WORLD_SIZE": str(world)})
    import torch.distributed as dist

    import platipy_amd as pa
    from tests.helpers import install_emu_runtime

    install_emu_runtime()
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        ids = ["001", "002", "003"]
        target, _, _, atlases = _data(pa, ids)
        mine = {k: v for k, v in atlases.items() if k in ids[rank::world]}   # a rank only needs its own share
        results, prob = pa.projects.multiatlas.run_segmentation(target, _settings(ids), atlases=mine)
        # every atlas holds both structures: the fusion all_reduce carries [sum w, sum w L_1, sum w L_2] = 1 + S volumes
        crop_voxels = pa.projects.multiatlas.run_segmentation.last_fusion_payload_bytes // (4 * 3)
        assert pa.projects.multiatlas.run_segmentation.last_fusion_payload_bytes == 3 * 4 * crop_voxels and crop_voxels > 1000
        np.save(os.path.join(out_dir, f"wh_{rank}.npy"), results["WHOLEHEART"].numpy())
        np.save(os.path.join(out_dir, f"prob_{rank}.npy"), prob["WHOLEHEART"].numpy())
        # every exchange is timed under its label (bench.py's N > 1 line reports them)
        ms = pa.projects.multiatlas.run_segmentation.last_exchange_ms
        assert {"crop_allreduce", "fusion_allreduce", "fusion_layout"} <= set(ms) and all(v >= 0.0 for v in ms.values()), ms
        assert pa.projects.multiatlas.run_segmentation.last_world_size == world
        # the same job with the sums reduced onto rank 0 only (north_star's "RCCL reduce"): rank 0 gets the identical
        # result, the other rank an empty one
        r2, p2 = pa.projects.multiatlas.run_segmentation(target, _settings(ids), atlases=mine, fusion_collective="reduce")
        ms2 = pa.projects.multiatlas.run_segmentation.last_exchange_ms
        assert "fusion_reduce" in ms2 and "fusion_allreduce" not in ms2
        if rank == 0:
            assert np.array_equal(r2["WHOLEHEART"].numpy(), results["WHOLEHEART"].numpy())
            assert np.array_equal(p2["WHOLEHEART"].numpy(), prob["WHOLEHEART"].numpy())
        else:
            assert r2 == {} and p2 == {}
    finally:
        dist.destroy_process_group()


@pytest.mark.slow
def test_run_segmentation_two_ranks_gloo(tmp_path):
    """world_size 2 over gloo on the CPU: ranks split the atlases, the fusion all_reduce makes every rank hold the
    same result, and that result equals the single-process run (fp32 sums in a different order: probabilities within
    1e-5, masks identical)."""
    import torch.multiprocessing as mp

    import platipy_amd as pa
    from tests.helpers import install_emu_runtime

    port = 29500 + (os.getpid() % 2000)
    mp.spawn(_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    wh0, wh1 = np.load(tmp_path / "wh_0.npy"), np.load(tmp_path / "wh_1.npy")
    p0, p1 = np.load(tmp_path / "prob_0.npy"), np.load(tmp_path / "prob_1.npy")
    np.testing.assert_array_equal(wh0, wh1)
    np.testing.assert_array_equal(p0, p1)
    # single-process reference
    from platipy_amd import runtime

    saved = (runtime.context, runtime.default_device)
    try:
        install_emu_runtime()
        ids = ["001", "002", "003"]
        target, tmask, _, atlases = _data(pa, ids)
        results, prob = pa.projects.multiatlas.run_segmentation(target, _settings(ids), atlases=atlases)
    finally:
        runtime.context, runtime.default_device = saved
    np.testing.assert_allclose(p0, prob["WHOLEHEART"].numpy(), rtol=0, atol=1e-5)
    np.testing.assert_array_equal(wh0, results["WHOLEHEART"].numpy())
    assert dice(wh0, tmask) > 0.93


def _iar_case(pa):
    """Seven small atlases (wobbly spheres, one of them displaced) with their CT images, and a target."""
    from tests.helpers import smooth_noise

    shape, sp = (22, 30, 34), (1.0, 1.0, 2.0)
    rng = np.random.default_rng(21)
    zz, yy, xx = np.meshgrid(*[np.arange(n) for n in shape], indexing="ij")
    target = pa.image_from_array(rng.normal(0, 40, shape).astype(np.float32), sp, (0, 0, 0))
    ids = [f"{i:02d}" for i in range(7)]
    aset = {}
    for k, cid in enumerate(ids):
        r = 8 + 1.0 * smooth_noise(shape, 700 + k, cells=4)
        m = ((zz - 11) ** 2 + (yy - 15) ** 2 + (xx - 17) ** 2 <= r ** 2).astype(np.uint8)
        if k == 5:
            m = np.roll(m, (0, 6, -5), axis=(0, 1, 2))
        ct = (target.numpy() + rng.normal(0, 10 + 3 * k, shape)).astype(np.float32)
        aset[cid] = {"DIR": {"CT Image": pa.image_from_array(ct, sp, (0, 0, 0)), "HEART": pa.image_from_array(m, sp, (0, 0, 0))}}
    return target, ids, aset


def _iar_worker(rank, world, port, out_dir):
    os.environ.update({"MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port), "RANK": str(rank), "WORLD_SIZE": str(world)})
    import torch.distributed as dist

    import platipy_amd as pa
    from platipy_amd.label.iar import run_iar_distributed
    from platipy_amd.projects import multiatlas
    from tests.helpers import install_emu_runtime

    install_emu_runtime()
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        target, ids, aset = _iar_case(pa)
        my_ids = ids[rank::world]                                   # 7 atlases on 2 ranks: the last slot is half empty
        weights = {i: float(pa.label.compute_weight_map(target, aset[i]["DIR"]["CT Image"], vote_type="global").tensor.flatten()[0])
                   for i in my_ids}
        kept = run_iar_distributed(multiatlas._Dist(), {i: aset[i] for i in my_ids}, my_ids, ids, "HEART", target, weights,
                                   min_best_atlases=3, z_score_statistic="mad", outlier_method="iqr", outlier_factor=1.5)
        q = run_iar_distributed.last_q_results
        np.save(os.path.join(out_dir, f"kept_{rank}.npy"), np.array(kept))
        np.save(os.path.join(out_dir, f"q_{rank}.npy"), np.array([q[k] for k in sorted(q)]))
    finally:
        dist.destroy_process_group()


def test_distributed_iar_two_ranks_gloo(tmp_path, monkeypatch):
    """Atlas selection with the atlases spread over two ranks (gloo, CPU): both ranks take the decision the
    single-process run_iar takes on all atlases, from the same Q values."""
    import torch.multiprocessing as mp

    import platipy_amd as pa
    from platipy_amd.label import iar
    from tests.helpers import install_emu_runtime

    port = 31500 + (os.getpid() % 2000)
    mp.spawn(_iar_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    kept0, kept1 = np.load(tmp_path / "kept_0.npy"), np.load(tmp_path / "kept_1.npy")
    assert list(kept0) == list(kept1)
    np.testing.assert_array_equal(np.load(tmp_path / "q_0.npy"), np.load(tmp_path / "q_1.npy"))
    install_emu_runtime(lambda obj, name, value: monkeypatch.setattr(obj, name, value, raising=False))
    target, ids, aset = _iar_case(pa)
    for i in ids:
        aset[i]["DIR"]["Weight Map"] = pa.label.compute_weight_map(target, aset[i]["DIR"]["CT Image"], vote_type="global")
    single = iar.run_iar(atlas_set=aset, reference_structure="HEART", min_best_atlases=3, z_score_statistic="mad", outlier_method="iqr",
                         outlier_factor=1.5)
    assert list(single) == list(kept0)
    assert "05" not in kept0 and len(kept0) >= 3                       # the displaced contour went


def test_run_segmentation_with_iterative_atlas_removal(host_api):
    """Config 5's "iterative atlas selection": an atlas whose label is grossly wrong is dropped before fusion."""
    pa = host_api
    from tests.helpers import smooth_noise

    ids = [f"{i:03d}" for i in range(1, 7)]
    target, tmask, _, atlases = _data(pa, ids)
    for k, cid in enumerate(ids):       # observers differ: wobble every atlas contour by about a voxel (identical contours make
        ct, m, _, sp = sphere_case(k)   # the reference's MAD z-scores 0/0)
        zz, yy, xx = np.meshgrid(*[np.arange(n) for n in m.shape], indexing="ij")
        r = 12 + 1.2 * smooth_noise(m.shape, 500 + k, cells=5)
        wob = ((zz - (15 + k)) ** 2 + (yy - (32 + k)) ** 2 + (xx - 32) ** 2 <= r ** 2).astype(np.uint8)
        atlases[cid]["WHOLEHEART"] = pa.image_from_array(wob, sp, ORIGIN)
    bad = ids[-1]
    wrong = np.roll(atlases[bad]["WHOLEHEART"].numpy(), (0, 14, -12), axis=(0, 1, 2))      # label far from where the CT says
    atlases[bad]["WHOLEHEART"] = pa.image_from_array(wrong, atlases[bad]["CT Image"].spacing, ORIGIN)
    st = _settings(ids)
    st["atlas_settings"]["atlas_structure_list"] = ["WHOLEHEART"]
    st["iar_settings"].update({"reference_structure": "WHOLEHEART", "min_best_atlases": 3})
    res, _ = pa.projects.multiatlas.run_segmentation(target, st, atlases=atlases)
    removed = pa.projects.multiatlas.run_segmentation.last_iar_removed
    assert bad in removed and len(removed) <= 3          # the IQR fence on six atlases may also drop a borderline one
    assert dice(res["WHOLEHEART"].numpy(), tmask) > 0.9


def test_fusion_payload_with_a_structure_missing_from_one_atlas(host_api):
    """An atlas without a structure does not vote on it (fusion.py:263-276): the weight sums then differ per structure and
    the exchange buffer falls back to 2 S volumes; the probabilities equal combine_labels' on the same atlases."""
    pa = host_api
    ids = ["001", "002", "003"]
    target, tmask, tsub, atlases = _data(pa, ids)
    del atlases["002"]["SUBSTRUCTURE"]
    results, prob = pa.projects.multiatlas.run_segmentation(target, _settings(ids), atlases=atlases)
    nbytes = pa.projects.multiatlas.run_segmentation.last_fusion_payload_bytes
    assert nbytes % (4 * 4) == 0                                   # 2 S = 4 volumes
    assert dice(results["WHOLEHEART"].numpy(), tmask) > 0.93 and dice(results["SUBSTRUCTURE"].numpy(), tsub) > 0.5


def test_shared_weight_sum_fusion_on_an_odd_voxel_count(host_api, monkeypatch):
    """Every atlas carries every structure: the fusion buffer is [sum w, sum w L_1 .. sum w L_3], structures 2 and 3
    accumulate with wsum = NULL, and with 7 x 9 x 11 = 693 voxels (2772 bytes a volume) every row after the first sits off
    16-byte alignment, so the accumulation runs on the 4-byte arm of the map kernel.  The registrations are replaced by the
    identity (a volume this small is below their pyramids; they are not what is tested), the fusion step runs as shipped, and
    its probabilities equal combine_labels' on the same propagated atlases, structure by structure."""
    pa = host_api
    from platipy_amd.projects import multiatlas as M
    from tests.helpers import smooth_noise

    shape, spacing = (7, 9, 11), (1.0, 1.2, 2.0)
    rng = np.random.default_rng(5)
    ct = (40.0 * smooth_noise(shape, 300, cells=3) + rng.normal(0, 5, shape)).astype(np.float32)
    names = ["A", "B", "C"]
    ids = ["001", "002", "003"]
    atlases = {}
    for k, cid in enumerate(ids):
        entry = {"CT Image": pa.image_from_array((ct + 10.0 * smooth_noise(shape, 310 + k, cells=3)).astype(np.float32), spacing, ORIGIN)}
        for j, s in enumerate(names):
            entry[s] = pa.image_from_array((smooth_noise(shape, 320 + 3 * k + j, cells=3) > 0.1 * j).astype(np.uint8), spacing, ORIGIN)
        atlases[cid] = entry
    target = pa.image_from_array(ct, spacing, ORIGIN)
    monkeypatch.setattr(M, "linear_registration", lambda fixed, moving, **kw: (moving, None))
    monkeypatch.setattr(M, "fast_symmetric_forces_demons_registration", lambda fixed, moving, **kw: (moving, None, None))
    monkeypatch.setattr(M, "apply_transform", lambda image, *a, **kw: image)
    monkeypatch.setattr(M, "label_to_roi", lambda label, expansion_mm=None: (list(target.GetSize()), [0, 0, 0]))
    st = _settings(ids)
    st["atlas_settings"]["atlas_structure_list"] = names
    _, prob, atlas_set = M.run_segmentation(target, st, atlases=atlases, return_atlas_set=True)
    n = int(np.prod(shape))
    assert n % 4 == 1 and M.run_segmentation.last_fusion_payload_bytes == (1 + len(names)) * n * 4      # the shared-sum layout
    for s in names:
        want = pa.label.fusion.combine_labels(atlas_set, s, label="DIR")[s].numpy()
        got = prob[s].numpy()
        assert want.max() == 1.0 and 0 < (want > 0).sum()
        print(s, "max |difference|", np.abs(got - want).max())
        np.testing.assert_allclose(got, want, rtol=0, atol=5e-6)


def _contours_worker(rank, world, port, out_dir):
    os.environ.update({"MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port), "RANK": str(rank), "WORLD_SIZE": str(world)})
    import torch.distributed as dist

    import platipy_amd as pa
    from tests.helpers import install_emu_runtime
    from tests.test_cardiac import _reference_test_settings, cardiac_data

    install_emu_runtime()
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        data = cardiac_data(pa, 2)
        cases = list(data.keys())
        st = _reference_test_settings(pa, cases, out_dir, ["WHOLEHEART"], False)
        st["return_proba_as_contours"] = True
        atl = {c: {"CT Image": data[c]["CT"], "WHOLEHEART": data[c]["WHOLEHEART"]} for c in cases[:-1][rank::world]}
        out, prob = pa.projects.cardiac.run_cardiac_segmentation(data[cases[-1]]["CT"], settings=st, atlases=atl)
        np.save(os.path.join(out_dir, f"enc_{rank}.npy"), prob["WHOLEHEART"].numpy())
    finally:
        dist.destroy_process_group()


@pytest.mark.slow
def test_return_proba_as_contours_two_ranks_gloo(tmp_path, monkeypatch):
    """cardiac/run.py:945-970 with the atlases spread over two ranks: every rank ends with the image that encodes atlas
    k's contour in bit k + 1 (one integer all_reduce of disjoint bit sets), equal to the single-process encoding."""
    import torch.multiprocessing as mp

    import platipy_amd as pa
    from tests.helpers import install_emu_runtime
    from tests.test_cardiac import _reference_test_settings, cardiac_data

    port = 36500 + (os.getpid() % 2000)
    mp.spawn(_contours_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    e0, e1 = np.load(tmp_path / "enc_0.npy"), np.load(tmp_path / "enc_1.npy")
    np.testing.assert_array_equal(e0, e1)
    install_emu_runtime(lambda obj, name, value: monkeypatch.setattr(obj, name, value, raising=False))
    data = cardiac_data(pa, 2)
    cases = list(data.keys())
    st = _reference_test_settings(pa, cases, tmp_path, ["WHOLEHEART"], False)
    st["return_proba_as_contours"] = True
    atl = {c: {"CT Image": data[c]["CT"], "WHOLEHEART": data[c]["WHOLEHEART"]} for c in cases[:-1]}
    _, prob = pa.projects.cardiac.run_cardiac_segmentation(data[cases[-1]]["CT"], settings=st, atlases=atl)
    single = prob["WHOLEHEART"].numpy()
    np.testing.assert_array_equal(e0, single)
    assert set(np.unique(single)) - {0} and (single & 0b11110).max() > 0        # bits 1..4 = the four atlases
