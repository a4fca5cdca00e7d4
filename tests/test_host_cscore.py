"""Host logic of the C-score drop-in on CPU: SPair-71k loader vs the reference loader's output, eval() aggregation vs the
reference's eval() on a mini tree (tests/golden/mini_spair + spair_host.npz, produced by running the reference), pair
sharding + all-reduce on 2 gloo ranks.  The two device entry points are replaced by oracle-backed CPU stand-ins through
monkeypatching — the oracle is the checker, the product has no CPU fallback."""
import argparse
import os
import shutil

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from law_of_vision_representation_in_mllms_amd import cscore_ops
from law_of_vision_representation_in_mllms_amd.C_score import pck_train as PT
from law_of_vision_representation_in_mllms_amd.C_score import pck_train_two as PT2
from law_of_vision_representation_in_mllms_amd.C_score.utils import utils_dataset as UD
from oracle import cscore as OC

G = os.path.join(os.path.dirname(__file__), "golden")
CATS = ("aeroplane", "cat")


def cpu_descriptors(m, P, split=0, layout="cp"):
    """[C, P^2] (or position-major [P^2, C]) raw map -> [1, P^2, C] descriptors, one encoder (pck_train.py) or two (pck_train_two.py)."""
    if layout == "pc":
        m = m.t()
    C = m.shape[0]
    if split == 0:
        return OC.descriptors_from_map(m.view(1, C, P, P), P)
    return OC.normalize_feats_two(m.view(1, C, P * P).permute(0, 2, 1), split)


def cpu_transfer(bank, img1, img2, patch_idx, nkp, P, window=5, soft_eval=True, beta=0.02, anno_size=840, split=0, layout="cp", sort_pairs=True, packed=None):
    n, kmax = patch_idx.shape
    out = torch.zeros(n, kmax, 2)
    for i in range(n):
        d1 = cpu_descriptors(bank[int(img1[i])], P, split, layout)
        d2 = cpu_descriptors(bank[int(img2[i])], P, split, layout)
        k = int(nkp[i])
        out[i, :k] = OC.keypoint_transfer(d1, d2, patch_idx[i, :k].numpy(), P, anno_size, soft_eval, window, beta)
    return out


def cpu_pck_counts(xy, kps1, kps2, thresholds, nkp, alphas=(0.1, 0.05, 0.01)):
    n = xy.shape[0]
    cnt = torch.zeros(n, 4, dtype=torch.int32)
    for i in range(n):
        k = int(nkp[i])
        _, nv, hits = OC.pair_pck(xy[i, :k], kps1[i, :k], kps2[i, :k], float(thresholds[i]), alphas)
        cnt[i, :3] = hits.sum(dim=1).int()
        cnt[i, 3] = nv
    return cnt


def cpu_mutual_nn(bank, img1, img2, P, chunk=2048, eps=1e-10):
    """oracle-backed stand-in of cscore_ops.mutual_nn_distance: position-major raw maps [n, P^2, C]"""
    out = []
    for a, b in zip(img1.tolist(), img2.tolist()):
        out.append(OC.mutual_nn_distance(OC.normalize_feats(bank[a][None].float()), OC.normalize_feats(bank[b][None].float())))
    return torch.stack(out)


@pytest.fixture
def cpu_ops(monkeypatch):
    monkeypatch.setattr(PT, "device", "cpu")              # pck_train picks cuda when a GPU is visible: the stand-ins take host tensors
    monkeypatch.setattr(cscore_ops, "transfer", cpu_transfer)
    monkeypatch.setattr(cscore_ops, "pck_counts", cpu_pck_counts)
    monkeypatch.setattr(cscore_ops, "mutual_nn_distance", cpu_mutual_nn)


def make_tree(tmp):
    z = np.load(f"{G}/spair_host.npz")
    root = os.path.join(tmp, "data", "SPair-71k")
    shutil.copytree(f"{G}/mini_spair", root)
    for key in z.files:
        if key.startswith("feat."):
            _, cat, i = key.split(".")
            os.makedirs(f"{root}/features/{cat}", exist_ok=True)
            torch.save(torch.from_numpy(z[key]), f"{root}/features/{cat}/img{i}_dino.pt")
        if key.startswith("feat2."):
            _, cat, i = key.split(".")
            os.makedirs(f"{root}/features/{cat}", exist_ok=True)
            torch.save(torch.from_numpy(z[key]), f"{root}/features/{cat}/img{i}_clip.pt")
    return root, z


def eval_args(root, P):
    return argparse.Namespace(NUM_PATCHES=P, COMPUTE_GEOAWARE_METRICS=False, ADAPT_FLIP=False, EVAL_DATASET="spair",
                              TRAIN_DATASET="spair", ANNO_SIZE=840, ENSEMBLE=1, MODEL="dino", SOFT_EVAL=True, SOFT_EVAL_WINDOW=5,
                              KPT_RESULT=False, TOTAL_SAVE_RESULT=0, MUTUAL_NN=False, TEST_SAMPLE=0, BBOX_THRE=True, DATA_DIR=root)


def eval_args_two(root, P):
    a = eval_args(root, P)
    del a.MODEL
    a.MODEL1, a.MODEL2, a.DUMMY_NET = "dino", "clip", True
    return a


def test_spair_loader_matches_reference():
    z = np.load(f"{G}/spair_host.npz")
    root = f"{G}/mini_spair"
    for cat in CATS:
        files, kps, thr, used = UD.load_spair_data(root, size=840, category=cat, split="test", subsample=0)
        assert [os.path.relpath(f, root) for f in files] == list(z[f"{cat}.files"])
        assert torch.equal(kps, torch.from_numpy(z[f"{cat}.kps"]))
        np.testing.assert_array_equal(np.asarray(thr, np.float64), z[f"{cat}.thr"])
        np.testing.assert_array_equal(used.numpy(), z[f"{cat}.used"])


def test_eval_matches_reference_eval(tmp_path, cpu_ops):
    root, z = make_tree(str(tmp_path))
    P, C = z["meta"].tolist()
    pck_010, pck_005, pck_001, results = PT.eval(eval_args(root, P), PT.DummyAggregationNetwork(), str(tmp_path), split="test")
    np.testing.assert_allclose([pck_010, pck_005, pck_001], z["eval.pck"], atol=1e-7)
    pred = np.stack([r["src_kpts_pred"] for r in results])
    np.testing.assert_allclose(pred, z["eval.pred"], atol=2e-3)
    assert results[0]["src_fn"].endswith(".jpg") and results[0]["resize_resolution"] == 840


def test_two_encoder_eval_matches_reference_eval(tmp_path, cpu_ops):
    """pck_train_two.py: separate per-encoder normalisation, concat, renormalise - against the reference's own eval()."""
    root, z = make_tree(str(tmp_path))
    P, C = z["meta"].tolist()
    pck_010, pck_005, pck_001, results = PT2.eval(eval_args_two(root, P), PT2.DummyAggregationNetwork(), str(tmp_path), split="test")
    np.testing.assert_allclose([pck_010, pck_005, pck_001], z["eval2.pck"], atol=1e-7)
    pred = np.stack([r["src_kpts_pred"] for r in results])
    np.testing.assert_allclose(pred, z["eval2.pred"], atol=2e-3)
    assert not np.allclose(z["eval2.pred"], z["eval.pred"], atol=1.0)       # the second encoder does change the answer


def test_two_encoder_normalize_feats_is_the_oracles():
    g = torch.Generator().manual_seed(5)
    a, b = torch.randn(1, 49, 20, generator=g) * 4, torch.randn(1, 49, 12, generator=g) * 0.1
    args = argparse.Namespace(DUMMY_NET=True)
    torch.testing.assert_close(PT2.normalize_feats(args, a, b), OC.normalize_feats_two(torch.cat([a, b], -1), 20), rtol=0, atol=1e-7)
    with pytest.raises(NotImplementedError):
        PT2.normalize_feats(argparse.Namespace(DUMMY_NET=False), a, b)
    a2 = PT2.parse_args(["--config", os.path.join(os.path.dirname(PT2.__file__), "configs", "eval_zero_shot_spair_two.yaml")])
    assert (a2.MODEL1, a2.MODEL2, a2.NUM_PATCHES, a2.DUMMY_NET) == ("clip", "sd1.5", 24, True)


def test_unsupported_modes_fail_loudly(tmp_path, cpu_ops):
    root, z = make_tree(str(tmp_path))
    a = eval_args(root, 16)
    a.ADAPT_FLIP = True                                              # no `_flip.pt` features in this tree: the reference's torch.load fails the same way
    with pytest.raises(FileNotFoundError, match="_dino_flip.pt"):
        PT.eval(a, PT.DummyAggregationNetwork(), str(tmp_path), split="test")
    a.ADAPT_FLIP, a.TOTAL_SAVE_RESULT = False, 5                      # qualitative PNGs of the first pairs: not built, says so
    with pytest.raises(NotImplementedError, match="TOTAL_SAVE_RESULT"):
        PT.eval(a, PT.DummyAggregationNetwork(), str(tmp_path), split="test")


def _worker(rank, world, tmp, port, q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    cscore_ops.transfer, cscore_ops.pck_counts = cpu_transfer, cpu_pck_counts
    PT.device = "cpu"
    root = os.path.join(tmp, "data", "SPair-71k")
    a = eval_args(root, 16)
    a.COMPUTE_GEOAWARE_METRICS = True                       # the geo-aware counters ride in the same all-reduce
    scores = []
    spy = lambda *args, **kw: (lambda r: (scores.append(r[1]), r)[1])(PT.compute_pck(*args, **kw))
    res = PT.eval(a, PT.DummyAggregationNetwork(), tmp, split="test", _compute=spy)
    q.put((rank, res[:3], np.stack([r["src_kpts_pred"] for r in res[3]]), np.array(scores, np.float64)))
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_pair_sharding_equals_reference(tmp_path):
    root, z = make_tree(str(tmp_path))
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 31500 + os.getpid() % 2000
    procs = [ctx.Process(target=_worker, args=(r, 2, str(tmp_path), port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = [q.get(timeout=180) for _ in range(2)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, pcks, pred, geo_scores in got:
        np.testing.assert_allclose(geo_scores, z["geo.scores"], rtol=0, atol=1e-12)
        np.testing.assert_allclose(pcks, z["eval.pck"], atol=1e-7)
        np.testing.assert_allclose(pred, z["eval.pred"], atol=2e-3)


def test_geo_aware_tables_are_the_references():
    import json
    from law_of_vision_representation_in_mllms_amd.C_score.utils import utils_geoware as UG
    z = np.load(f"{G}/spair_host.npz")
    assert UG.SPAIR_GEO_AWARE == json.loads(str(z["geo.table.spair"]))
    assert UG.AP10K_GEO_AWARE == json.loads(str(z["geo.table.ap10k"]))
    assert UG.renumber_indices([[4, 5], 9, [11]], counter=[0]) == [[0, 1], 2, [3]]
    assert UG.filtered_groups([0, [4, 5], [6, 7], 9], [0, 5, 6, 7]) == [[0], [1], [2, 3]]
    assert UG.geo_aware_points([[0], [1, 2], [3, 4]], [1, 1, 0, 1, 1], [1, 1, 1, 1, 0]) == [1]


@pytest.mark.parametrize("tag,kpt", [("geo", False), ("geokpt", True)])
def test_geo_aware_eval_matches_reference_eval(tmp_path, cpu_ops, caplog, tag, kpt):
    """COMPUTE_GEOAWARE_METRICS: geo_score per category, the weighted numbers and every geo log line of the reference's run."""
    import logging
    root, z = make_tree(str(tmp_path))
    P, C = z["meta"].tolist()
    a = eval_args(root, P)
    a.COMPUTE_GEOAWARE_METRICS, a.KPT_RESULT = True, kpt
    scores = []
    orig = PT.compute_pck

    def spy(*args, **kw):
        r = orig(*args, **kw)
        scores.append(r[1])
        return r
    with caplog.at_level(logging.INFO, logger="visrep.cscore"):
        p = PT.eval(a, PT.DummyAggregationNetwork(), str(tmp_path), split="test", _compute=spy)
    np.testing.assert_allclose(p[:3], z[f"{tag}.pck"], atol=1e-7)
    np.testing.assert_allclose(np.array(scores, np.float64), z[f"{tag}.scores"], rtol=0, atol=1e-12)
    ours = [m for m in caplog.messages if "geo" in m.lower()]
    assert ours == list(z[f"{tag}.log"])


def test_result_postprocessing_matches_reference(tmp_path, cpu_ops):
    """utils/eval_spair.py on the result list: per-image / per-keypoint PCK, all points and geometry-aware ones."""
    from law_of_vision_representation_in_mllms_amd.C_score.utils import eval_spair as ES
    root, z = make_tree(str(tmp_path))
    P, C = z["meta"].tolist()
    results = PT.eval(eval_args(root, P), PT.DummyAggregationNetwork(), str(tmp_path), split="test")[3]
    conv = ES.convert_all_results(results)
    img = np.concatenate([ES.get_img_result(conv)[0].numpy(), ES.get_img_result(conv, geo=True)[0].numpy(),
                          ES.get_img_result(conv, cls="cat", geo=True)[0].numpy()])
    std = np.concatenate([ES.get_std_result(conv)[0].numpy(), ES.get_std_result(conv, geo=True)[0].numpy()])
    n = [ES.get_img_result(conv)[1], ES.get_img_result(conv, geo=True)[1], ES.get_std_result(conv)[1], ES.get_std_result(conv, geo=True)[1]]
    np.testing.assert_allclose(img, z["post.img"], atol=1e-7)
    np.testing.assert_allclose(std, z["post.std"], atol=1e-7)
    assert n == z["post.n"].tolist()
    assert ES.get_img_result(conv, cls="nope")[1] == 0
    # flip=True (eval_spair.py:164-175,333-336,364-367): the left/right-group key points, against the reference module on the same results
    import json
    zf = np.load(f"{G}/evalflip.npz")
    assert [r["flip_idx"] for r in conv] == json.loads(str(zf["flip_idx"]))
    stdf = np.concatenate([ES.get_std_result(conv, flip=True)[0].numpy(), ES.get_std_result(conv, cls="cat", flip=True)[0].numpy()])
    imgf = np.concatenate([ES.get_img_result(conv, flip=True)[0].numpy(), ES.get_img_result(conv, cls="aeroplane", flip=True)[0].numpy()])
    nf = [ES.get_std_result(conv, flip=True)[1], ES.get_std_result(conv, cls="cat", flip=True)[1], ES.get_img_result(conv, flip=True)[1],
          ES.get_img_result(conv, cls="aeroplane", flip=True)[1]]
    np.testing.assert_allclose(stdf, zf["std"], atol=1e-7)
    np.testing.assert_allclose(imgf, zf["img"], atol=1e-7)
    assert nf == zf["n"].tolist()


# ------------------------------------------------------------------------------------------------ ADAPT_FLIP (§8f N4)
def make_flip_tree(tmp):
    root, z = make_tree(tmp)
    zf = np.load(f"{G}/adaptflip.npz")
    for key in zf.files:
        if key.startswith("flipfeat."):
            _, cat, i = key.split(".")
            torch.save(torch.from_numpy(zf[key]), f"{root}/features/{cat}/img{i}_dino_flip.pt")
    return root, z, zf


def test_flip_helpers_and_distance_oracle_match_the_reference():
    from law_of_vision_representation_in_mllms_amd.C_score.utils import utils_geoware as UG
    zf = np.load(f"{G}/adaptflip.npz")
    flip_list = [0, [1, 2], 3, [4, 5, 6]]
    vis = [True, True, False, True, True, True, True]
    k = torch.tensor([[10., 20., 1.], [30., 40., 1.], [50., 60., 0.], [70., 80., 1.], [90., 100., 1.], [110., 120., 1.], [130., 140., 1.]])
    for mod in (UG, OC):
        assert mod.permute_indices(flip_list, None) == zf["perm.all"].tolist()
        assert mod.permute_indices(flip_list, vis) == zf["perm.vis"].tolist()
        np.testing.assert_array_equal(mod.flip_keypoints(k, 840, mod.permute_indices(flip_list, None)).numpy(), zf["flipkps"])
    for tag in ("d6", "d16"):
        n1 = OC.normalize_feats(torch.from_numpy(zf[f"{tag}.f1"])[None])
        n2 = OC.normalize_feats(torch.from_numpy(zf[f"{tag}.f2"])[None])
        assert abs(OC.mutual_nn_distance(n1, n2).item() - float(zf[f"{tag}.dist"])) < 1e-6
    # the permute list compute_pck derives for a category: table restricted to the used key points, renumbered (pck_train.py:82-94)
    assert UG.flip_permutation(UG.SPAIR_FLIP["cat"], [0, 1, 4, 5, 8], 5) == [[0, 1], [2, 3], [4]]
    assert UG.flip_permutation(UG.SPAIR_FLIP["bottle"], list(range(10)), 10) == UG.SPAIR_FLIP["bottle"]


def test_adapt_flip_eval_matches_reference_eval(tmp_path, cpu_ops):
    """pck_train.eval with ADAPT_FLIP + MUTUAL_NN on the mini tree (mirrored feature file per image) == the reference's own run:
    6 of the 10 pairs take the mirrored prediction there."""
    root, z, zf = make_flip_tree(str(tmp_path))
    a = eval_args(root, 16)
    a.ADAPT_FLIP, a.MUTUAL_NN = True, True
    p10, p05, p01, results = PT.eval(a, PT.DummyAggregationNetwork(), str(tmp_path), split="test")
    np.testing.assert_allclose([p10, p05, p01], zf["eval.pck"], atol=1e-7)
    np.testing.assert_allclose(np.stack([r["src_kpts_pred"] for r in results]), zf["eval.pred"], atol=2e-3)
    assert not np.allclose(zf["eval.pred"], z["eval.pred"], atol=1.0)          # the flip branch really changes predictions
    a.MUTUAL_NN = False                                              # the mask-based distance without `_mask.png` files: None masks, as in the reference
    with pytest.raises(AttributeError, match="unsqueeze"):
        PT.eval(a, PT.DummyAggregationNetwork(), str(tmp_path), split="test")


def test_mask_distance_oracle_matches_the_reference():
    """oracle.cscore.masked_nn_distance against utils_correspondence.get_distance run as it stands on 60 x 60 maps (tests/golden/maskdist.npz:
    two blob-mask cases and one with exact zeros inside the masks - the `== 0 -> -100000` line compares elementwise)."""
    z = np.load(f"{G}/maskdist.npz")
    for tag in ("a", "b", "zeros"):
        f1, f2 = (torch.from_numpy(z[f"{tag}.{k}"].astype(np.float32))[None] for k in ("f1", "f2"))
        m1, m2 = (torch.from_numpy(z[f"{tag}.{k}"].astype(np.float32)) for k in ("m1", "m2"))
        want = float(z[f"{tag}.dist"])
        assert abs(OC.masked_nn_distance(f1, f2, m1, m2).item() - want) <= 1e-6 * abs(want), tag
    assert torch.isnan(OC.masked_nn_distance(f1, f2, torch.zeros(8, 8), m2))          # an empty source mask: the mean of nothing


def write_masks(root, cats, seed=5):
    """`<img>_mask.png` / `<img>_mask_flip.png` next to the features: one blob per image (PIL 'L' files, > 127 inside)."""
    from PIL import Image
    rs = np.random.RandomState(seed)
    for cat, n_img in cats.items():
        for i in range(n_img):
            for suffix in ("", "_flip"):
                yy, xx = np.mgrid[0:48, 0:64]
                cy, cx, ry, rx = rs.uniform(16, 32), rs.uniform(20, 44), rs.uniform(8, 20), rs.uniform(10, 26)
                m = ((((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2) <= 1).astype(np.uint8) * 255
                Image.fromarray(m, "L").save(f"{root}/features/{cat}/img{i}_mask{suffix}.png")


def masked_flip_expectation(root, a, z, zf, cats, dist_fn):
    """What pck_train.py:101-126 computes for the mini tree with ADAPT_FLIP and the mask-based distance, composed from the oracle's pieces."""
    from law_of_vision_representation_in_mllms_amd.C_score.utils import utils_geoware as UG
    from law_of_vision_representation_in_mllms_amd.C_score.utils.utils_dataset import load_eval_data
    from PIL import Image
    P = a.NUM_PATCHES
    preds, flips = [], 0
    mask = lambda cat, i, fl: (torch.from_numpy(np.array(Image.open(f"{root}/features/{cat}/img{i}_mask{'_flip' if fl else ''}.png").convert('L'))) > 127).float()
    for cat in cats:
        files, kps, thresholds, used = load_eval_data(a, root, cat, "test")
        permute_list = UG.flip_permutation(UG.SPAIR_FLIP[cat], used.tolist(), kps.shape[1])
        num = lambda f: int(os.path.basename(f)[3:-4])
        for n in range(len(files) // 2):
            i, j = num(files[2 * n]), num(files[2 * n + 1])
            k1, k2 = kps[2 * n].float(), kps[2 * n + 1].float()
            d1 = OC.descriptors_from_map(torch.from_numpy(z[f"feat.{cat}.{i}"]), P)
            d1f = OC.descriptors_from_map(torch.from_numpy(zf[f"flipfeat.{cat}.{i}"]), P)
            d2 = OC.descriptors_from_map(torch.from_numpy(z[f"feat.{cat}.{j}"]), P)
            vis = k1[:, 2] * k2[:, 2] > 0
            pred = OC.keypoint_transfer(d1, d2, OC.kpts_to_patch_idx(k1, P), P)
            kf = OC.flip_keypoints(k1, 840, OC.permute_indices(permute_list, vis))
            pred_f = OC.keypoint_transfer(d1f, d2, OC.kpts_to_patch_idx(kf, P), P)
            do, df = dist_fn(d1, d2, mask(cat, i, False), mask(cat, j, False)), dist_fn(d1f, d2, mask(cat, i, True), mask(cat, j, False))
            flips += int(df < do)
            preds.append((OC.adapt_flip_prediction(pred, pred_f, k1, k2, df, do, permute_list), used))
    return preds, flips


def test_adapt_flip_with_the_mask_distance_follows_the_oracle_chain(tmp_path, cpu_ops, monkeypatch):
    """ADAPT_FLIP without MUTUAL_NN (pck_train.py:122-124 -> get_distance) through pck_train.eval on the mini tree with mask files, the
    distance hook on the oracle (the product's is the device kernel: tests/test_gpu_dropin.py runs the same tree through it)."""
    root, z, zf = make_flip_tree(str(tmp_path))
    cats = {"aeroplane": 4, "cat": 3}
    write_masks(root, cats)
    monkeypatch.setattr(cscore_ops, "masked_nn_distance", lambda a_, b_, m1, m2, resolution=64: OC.masked_nn_distance(a_.cpu(), b_.cpu(), m1, m2, resolution))
    a = eval_args(root, 16)
    a.ADAPT_FLIP, a.MUTUAL_NN = True, False
    p10, p05, p01, results = PT.eval(a, PT.DummyAggregationNetwork(), str(tmp_path), split="test")
    want, flips = masked_flip_expectation(root, a, z, zf, cats, lambda *x: OC.masked_nn_distance(*x).item())
    assert 0 < flips < len(want)                                     # both branches of optimized_kps_1_to_2 are taken
    got = np.stack([r["src_kpts_pred"] for r in results])
    assert got.shape[0] == len(want)
    for n, (w, used) in enumerate(want):                              # src_kpts_pred: rows renumbered to the 30 SPair key-point slots
        np.testing.assert_allclose(got[n][used.numpy()], w.numpy(), atol=2e-3, err_msg=str(n))


def test_pack_rows_packs_the_pairs_of_a_target_into_32_row_tiles():
    """cscore_ops.pack_rows (host half of the packed key-point transfer): every key point of every pair sits in exactly one tile row, a tile
    holds pairs of ONE target, at most 32 rows, pairs are never split, the groups of a target are consecutive; on an SPair-shaped list the
    tiles are > 75 % full (one tile per pair: 36 %)."""
    from law_of_vision_representation_in_mllms_amd import cscore_ops as CO
    rs = np.random.RandomState(5)
    n = 12234
    img1, img2 = rs.randint(0, 1800, n), rs.randint(0, 1800, n)
    nkp = rs.randint(3, 21, n)
    nkp[:50] = 0                                                          # pairs without key points take no row
    idx = rs.randint(0, 256, (n, 20))
    tab, tgt = CO.pack_rows(img1, img2, idx, nkp)
    assert tab.shape[1:] == (32, 4) and tab.dtype == np.int32 and len(tgt) == len(tab)
    used = tab[:, :, 0] >= 0
    assert used.sum() == nkp.sum() and used.mean() > 0.75
    seen = set()
    for g in range(len(tab)):
        rows = tab[g][used[g]]
        assert (used[g][: len(rows)]).all()                               # rows are filled from the top
        for z in np.unique(rows[:, 0]):
            r = rows[rows[:, 0] == z]
            assert img2[z] == tgt[g] and len(r) == nkp[z] and (r[:, 1] == np.arange(nkp[z])).all()       # whole pair, in key-point order
            assert (r[:, 2] == img1[z]).all() and (r[:, 3] == idx[z, : nkp[z]]).all()
            assert z not in seen
            seen.add(int(z))
    assert seen == set(np.nonzero(nkp)[0].tolist())
    assert (np.diff(tgt) >= 0).all()                                      # groups of one target are consecutive (and targets ascend)
    e_tab, e_tgt = CO.pack_rows(img1[:0], img2[:0], idx[:0], nkp[:0])
    assert e_tab.shape == (0, 32, 4) and e_tgt.shape == (0,)
