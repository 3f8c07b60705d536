"""On-disk dataset directories of 3d-beats, read side only.

Layout written by the reference's data generators (src/live_data_convert.py:287-298, 456-458) and read by
`DecisionTreeDatasetConfig` (src/decision_tree.py:21-122):

    <dir>/config.json            {"img_dims": [W, H], "num_images": N, "id_to_color": {"0": [0,0,0,0], "1": [r,g,b,255], ...}}
    <dir>/00000000_depth.png     16-bit depth, background already 65535
    <dir>/00000000_labels.png    16-bit class ids (0 = unlabelled)

This class keeps the reference's constructor, attributes and block getters so that harnesses such as
src/test_on_saved_model.py:44-56 run unchanged, but blocks are plain device arrays filled from the PNGs
(the reference stages them through nvcomp-compressed blocks, which is training-side machinery).
"""
import json
import os

import numpy as np

from .joint_votes import DEFAULT_MAX_VAR

# Not in the reference: joint targets beside a dataset's frames, int32 [num_images, J, 3] = (tx, ty, tz) per image and joint
# (rule V1 of include/rdf_labels.h), written by HandSceneRenderer.make_dataset(targets=True).  A directory without the file is
# a plain dataset.
TARGETS_FILE = 'targets.npy'
# Not in the reference either: the hand shape of every frame of a shape dataset, int32 [num_images], written by
# HandSceneRenderer.make_shape_dataset.
SHAPES_FILE = 'shapes.npy'


class DecisionTreeDatasetConfig:
    @staticmethod
    def multiple(dataset_dir, images):
        """Several datasets over one directory, e.g. [(n_train, per_block, 'train'), (n_test, None, 'test')]
        (decision_tree.py:24-44).  Like the reference, every part draws its own random subset."""
        with open(os.path.join(dataset_dir, 'config.json')) as fh:
            total_images = json.loads(fh.read())['num_images']
        assert sum(n for n, _, _ in images) <= total_images
        return tuple(DecisionTreeDatasetConfig(dataset_dir, num_images=n, images_per_block=(per_block or n),
                                               imgs_name=name) for n, per_block, name in images)

    def __init__(self, dataset_dir, num_images=0, images_per_block=0, imgs_name='data0', shuffle=True):
        self.dataset_dir = dataset_dir
        with open(os.path.join(dataset_dir, 'config.json')) as fh:
            cfg = json.loads(fh.read())
        self.cfg = cfg
        self.imgs_name = imgs_name

        self.img_dims = tuple(cfg['img_dims'])  # (x, y)
        self.id_to_color = {0: np.array([0, 0, 0, 0], dtype=np.uint8)}
        for i, c in cfg['id_to_color'].items():
            self.id_to_color[int(i)] = np.array(c, dtype=np.uint8)

        self.total_available_images = cfg['num_images']
        self.num_images = num_images
        if self.num_images == 0:
            return
        assert self.num_images <= self.total_available_images

        self.images_per_block = images_per_block or self.num_images
        assert self.num_images % self.images_per_block == 0
        self.num_image_blocks = self.num_images // self.images_per_block

        idxes = list(range(self.total_available_images))
        if shuffle:
            np.random.shuffle(idxes)   # the reference draws from the global numpy RNG (decision_tree.py:68)
        self.img_idxes = idxes[0:self.num_images]

    # -- reading -----------------------------------------------------------------------------
    def _load(self, img_idx, name):
        from PIL import Image
        path = os.path.join(self.dataset_dir, f'{str(img_idx).zfill(8)}_{name}.png')
        a = np.array(Image.open(path)).astype(np.uint16)
        assert a.shape == (self.img_dims[1], self.img_dims[0]), f'{path}: {a.shape}'
        return a

    def get_block_cpu(self, block_num, name):
        out = np.empty((self.images_per_block, self.img_dims[1], self.img_dims[0]), dtype=np.uint16)
        for j in range(self.images_per_block):
            out[j] = self._load(self.img_idxes[block_num * self.images_per_block + j], name)
        return out

    def get_depth_block_cu(self, block_num, arr_out):
        arr_out.set(self.get_block_cpu(block_num, 'depth'))

    def get_labels_block_cu(self, block_num, arr_out):
        arr_out.set(self.get_block_cpu(block_num, 'labels'))

    # -- bookkeeping (decision_tree.py:85-122) -------------------------------------------------
    def num_classes(self):
        return len(self.id_to_color)

    def num_pixels(self):
        return self.num_images * self.img_dims[0] * self.img_dims[1]

    def images_shape(self):
        return (self.num_images, self.img_dims[1], self.img_dims[0])

    def _palette(self):
        """(sorted RGBA keys as uint32, their class ids, id -> RGBA table) built once from id_to_color."""
        if getattr(self, "_pal", None) is None:
            ids = np.array(sorted(self.id_to_color), dtype=np.int64)
            rgba = np.stack([np.asarray(self.id_to_color[int(i)], dtype=np.uint8) for i in ids])
            keys = np.ascontiguousarray(rgba).view(np.uint32).reshape(-1)
            order = np.argsort(keys, kind="stable")
            table = np.zeros((int(ids.max()) + 1, 4), dtype=np.uint8)
            table[ids] = rgba
            self._pal = (keys[order], ids[order], table)
        return self._pal

    def convert_colors_to_ids(self, labels_color):
        """RGBA label image [H, W, 4] -> class ids [H, W] (decision_tree.py:97-110): every pixel must carry one of the
        dataset's colours.  One 32-bit key per pixel, looked up in the sorted palette."""
        keys, ids, _ = self._palette()
        px = np.ascontiguousarray(labels_color, dtype=np.uint8)
        assert px.shape == (self.img_dims[1], self.img_dims[0], 4), px.shape
        k = px.view(np.uint32).reshape(px.shape[0], px.shape[1])
        at = np.minimum(np.searchsorted(keys, k), keys.size - 1)
        assert np.array_equal(keys[at], k), 'every pixel must carry a known label colour'
        return ids[at].astype(np.uint16)

    def convert_ids_to_colors(self, labels_ids):
        """Class ids [N, H, W] -> RGBA [N, H, W, 4] (decision_tree.py:112-122); an id the dataset does not know stays
        transparent black."""
        n, y, x = labels_ids.shape
        assert (y, x) == (self.img_dims[1], self.img_dims[0])
        _, _, table = self._palette()
        ids = np.asarray(labels_ids).astype(np.int64)
        known = (ids >= 0) & (ids < table.shape[0])
        return np.where(known[..., None], table[np.where(known, ids, 0)], np.uint8(0)).astype(np.uint8)


def write_dataset(dataset_dir, depth, labels, id_to_color):
    """Writes a dataset directory in the layout above (used by tests and tools; data_convert.RecordingConverter
    writes the same layout from a recording, as the reference's live_data_convert.py does).  depth, labels: uint16 [N, H, W]; id_to_color: {id: [r, g, b, a]} without id 0."""
    from PIL import Image
    os.makedirs(dataset_dir, exist_ok=True)
    n, h, w = depth.shape
    cfg = {'img_dims': [int(w), int(h)], 'num_images': int(n), 'id_to_color': {'0': [0, 0, 0, 0]}}
    for k, c in id_to_color.items():
        cfg['id_to_color'][str(int(k))] = [int(v) for v in c]
    with open(os.path.join(dataset_dir, 'config.json'), 'w') as fh:
        fh.write(json.dumps(cfg))
    for i in range(n):
        Image.fromarray(np.ascontiguousarray(depth[i], dtype=np.uint16)).save(
            os.path.join(dataset_dir, f'{str(i).zfill(8)}_depth.png'))
        Image.fromarray(np.ascontiguousarray(labels[i], dtype=np.uint16)).save(
            os.path.join(dataset_dir, f'{str(i).zfill(8)}_labels.png'))


def read_targets(dataset_dir, images):
    """The joint targets of a dataset directory's images `images` (indices into the directory, e.g. a
    DecisionTreeDatasetConfig's img_idxes, in that order): host int32 [len(images), J, 3]."""
    path = os.path.join(dataset_dir, TARGETS_FILE)
    if not os.path.exists(path):
        raise FileNotFoundError(f"{dataset_dir} carries no joint targets ({TARGETS_FILE}): write it with "
                                "HandSceneRenderer.make_dataset(..., targets=True)")
    with open(os.path.join(dataset_dir, 'config.json')) as fh:
        total = json.loads(fh.read())['num_images']
    t = np.load(path)
    if t.dtype != np.int32 or t.ndim != 3 or t.shape[0] != total or t.shape[2] != 3:
        raise ValueError(f"{path}: int32 [{total}, J, 3] expected, found {t.dtype} {list(t.shape)}")
    idx = np.asarray(list(images), np.int64).reshape(-1)
    if idx.size and (idx.min() < 0 or idx.max() >= total):
        raise IndexError(f"images outside 0..{total - 1}")
    return np.ascontiguousarray(t[idx])


def read_shapes(dataset_dir, images):
    """The hand shapes of a shape dataset's images `images` (indices into the directory, e.g. a DecisionTreeDatasetConfig's
    img_idxes, in that order): host int32 [len(images)], indices into the `shapes` the directory was made with
    (HandSceneRenderer.make_shape_dataset); every hand pixel of image n carries the label 1 + shapes[n]."""
    path = os.path.join(dataset_dir, SHAPES_FILE)
    if not os.path.exists(path):
        raise FileNotFoundError(f"{dataset_dir} carries no hand shapes ({SHAPES_FILE}): write it with "
                                "HandSceneRenderer.make_shape_dataset")
    with open(os.path.join(dataset_dir, 'config.json')) as fh:
        total = json.loads(fh.read())['num_images']
    s = np.load(path)
    if s.dtype != np.int32 or s.shape != (total,):
        raise ValueError(f"{path}: int32 [{total}] expected, found {s.dtype} {list(s.shape)}")
    idx = np.asarray(list(images), np.int64).reshape(-1)
    if idx.size and (idx.min() < 0 or idx.max() >= total):
        raise IndexError(f"images outside 0..{total - 1}")
    return np.ascontiguousarray(s[idx])


def score_shape_model(model_path, dataset_dir, num_images, labels_reduce=1, **voter_settings):
    """A shape forest (train_forest on a make_shape_dataset directory) on `num_images` random images of a shape dataset,
    frame by frame: ShapeVoter.pool and .decide on the device, one read of the rows.  Returns a dict: `confusion` int64
    [C, C + 1], the frames by true class (1 + shape index; row 0 stays empty) and raw class, the last column the frames
    without a shape (raw -1); `accuracy`, the share of frames whose pooled SOFT vote names the true class; `accuracy_hard`,
    the same for the hard vote, the argmax of the pool's per-class counts of pixel labels (first greatest; a frame without a
    voting pixel counts as wrong); `frames`; `raw` and `truth`, int64 [frames], raw as decided and truth as a class.
    voter_settings: ShapeVoter's min_pixels and min_conf; `hold` plays no part, the held decision is not scored."""
    from .decision_tree import DecisionForest
    from .device import DeviceArray
    from .shape import ShapeVoter
    forest = DecisionForest.load(model_path)
    ds = DecisionTreeDatasetConfig(dataset_dir, num_images=num_images, imgs_name='test')
    n, h, w = ds.images_shape()
    depth = DeviceArray((n, h, w), np.uint16)
    ds.get_depth_block_cu(0, depth)
    truth = read_shapes(dataset_dir, ds.img_idxes).astype(np.int64) + 1
    voter = ShapeVoter(forest, (h, w), labels_reduce=labels_reduce, **voter_settings)
    C = voter.C
    pool_cu = voter.pool(depth)
    raw = voter.decide(pool_cu).get()[:, 0].astype(np.int64)
    pool = pool_cu.get()
    hard = np.where(pool[:, 2 * C] > 0, np.argmax(pool[:, C:2 * C], axis=1), -1)
    confusion = np.zeros((C, C + 1), np.int64)
    for t, r in zip(truth.tolist(), raw.tolist()):
        if 0 <= t < C:
            confusion[t, C if r < 0 else r] += 1
    return dict(confusion=confusion, accuracy=float(np.mean(raw == truth)) if n else float('nan'),
                accuracy_hard=float(np.mean(hard == truth)) if n else float('nan'), frames=int(n), raw=raw, truth=truth)


def evaluate_saved_model(model_path, dataset_dir, num_images, out_dir=None):
    """The accuracy harness of src/test_on_saved_model.py:23-67 without the GLFW window: returns
    `pct. matching pixels` = matches / labelled pixels, optionally saving colour renders."""
    from .decision_tree import DecisionForest, DecisionTreeEvaluator
    from .device import DeviceArray
    from .util import MAX_UINT16
    forest = DecisionForest.load(model_path)
    ev = DecisionTreeEvaluator()
    ds = DecisionTreeDatasetConfig(dataset_dir, num_images=num_images, imgs_name='test')
    depth = DeviceArray(ds.images_shape(), np.uint16)
    ds.get_depth_block_cu(0, depth)
    truth = DeviceArray(ds.images_shape(), np.uint16)
    ds.get_labels_block_cu(0, truth)
    truth_cpu = truth.get()
    out = DeviceArray(ds.images_shape(), np.uint16).fill(MAX_UINT16)
    ev.get_labels_forest(forest, depth, out)
    got = out.get()
    pct = float(np.sum(got == truth_cpu) / np.sum(truth_cpu > 0))
    if out_dir:
        from PIL import Image
        os.makedirs(out_dir, exist_ok=True)
        render = ds.convert_ids_to_colors(got)
        for i in range(ds.num_images):
            Image.fromarray(render[i]).save(os.path.join(out_dir, f'eval_labels_{str(i).zfill(8)}.png'))
    return pct


def score_saved_model(model_path, dataset_dir, num_images, labels_reduce=1):
    """evaluate_saved_model's flow with the comparison on the device: the forest's label maps of `num_images` random images
    against their truth as a score.Score (confusion matrix, per-class and per-image figures).  No label map is read back.
    With the same numpy seed, .pct_matching at labels_reduce 1 is evaluate_saved_model's return value bit for bit; above
    1 the forest writes [H // r, W // r] maps and the truth is sampled at (x * r, y * r)."""
    from .decision_tree import DecisionForest, DecisionTreeEvaluator
    from .device import DeviceArray
    from .score import LabelScorer
    from .util import MAX_UINT16
    forest = DecisionForest.load(model_path)
    ev = DecisionTreeEvaluator()
    ds = DecisionTreeDatasetConfig(dataset_dir, num_images=num_images, imgs_name='test')
    n, h, w = ds.images_shape()
    depth = DeviceArray((n, h, w), np.uint16)
    ds.get_depth_block_cu(0, depth)
    truth = DeviceArray((n, h, w), np.uint16)
    ds.get_labels_block_cu(0, truth)
    out = DeviceArray((n, h // labels_reduce, w // labels_reduce), np.uint16).fill(MAX_UINT16)
    ev.get_labels_forest(forest, depth, out, labels_reduce=labels_reduce)
    scorer = LabelScorer(max(int(forest.num_classes), ds.num_classes()))
    return scorer.add(out, truth, labels_reduce, per_image=True).result()


def calibrate_saved_model(model_path, dataset_dir, num_images, labels_reduce=1, bins=64):
    """score_saved_model's flow through ONE ungated posterior pass (DecisionTreeEvaluator.get_posteriors_forest, min_conf 0):
    returns (score.Score, score.Calibration) of the forest on `num_images` random images, read as score_saved_model reads
    them -- with the same numpy seed the Score is score_saved_model's.  The Calibration says how often a pixel of a given
    confidence is right, and picks a rejection threshold from that (Calibration.min_conf_for).  No map is read back."""
    from .decision_tree import DecisionForest, DecisionTreeEvaluator
    from .device import DeviceArray
    from .score import ConfidenceScorer, LabelScorer
    from .util import MAX_UINT16
    forest = DecisionForest.load(model_path)
    ev = DecisionTreeEvaluator()
    ds = DecisionTreeDatasetConfig(dataset_dir, num_images=num_images, imgs_name='test')
    n, h, w = ds.images_shape()
    depth = DeviceArray((n, h, w), np.uint16)
    ds.get_depth_block_cu(0, depth)
    truth = DeviceArray((n, h, w), np.uint16)
    ds.get_labels_block_cu(0, truth)
    out = DeviceArray((n, h // labels_reduce, w // labels_reduce), np.uint16).fill(MAX_UINT16)
    conf = DeviceArray(out.shape, np.uint16).fill(0)
    ev.get_posteriors_forest(forest, depth, out, conf, labels_reduce=labels_reduce)
    scorer = LabelScorer(max(int(forest.num_classes), ds.num_classes()))
    score = scorer.add(out, truth, labels_reduce, per_image=True).result()
    return score, ConfidenceScorer(bins).add(out, conf, truth, labels_reduce).result()


def score_layered_model(config_filename, dataset_dir, num_images, labels_reduce=2, scale_factor=1., min_conf=None):
    """Score a layered model -- what the app runs -- on `num_images` random images of a dataset: LayeredDecisionForest.run per
    frame into one [N, H // r, W // r] array of composite labels, scored in one pass against the truth sampled at
    (x * r, y * r).  The host comparison cannot do this: the shapes differ.  The dataset's ids must be the composite's.
    min_conf: the stack's per-layer confidence thresholds (LayeredDecisionForest.min_conf); None: plain labels."""
    from .decision_tree import LayeredDecisionForest
    from .device import DeviceArray
    from .engine.buffer import GpuBuffer
    from .score import LabelScorer
    ds = DecisionTreeDatasetConfig(dataset_dir, num_images=num_images, imgs_name='test')
    n, h, w = ds.images_shape()
    layered = LayeredDecisionForest.load(config_filename, (h, w), labels_reduce)
    layered.min_conf = min_conf
    hl, wl = layered.labels_dims
    depth = DeviceArray((n, h, w), np.uint16)
    ds.get_depth_block_cu(0, depth)
    truth = DeviceArray((n, h, w), np.uint16)
    ds.get_labels_block_cu(0, truth)
    composite = DeviceArray((n, hl, wl), np.uint16)
    depth_buf, labels_buf = GpuBuffer((h, w), dtype=np.uint16), GpuBuffer((hl, wl), dtype=np.uint16)
    for i in range(n):
        depth_buf.cu().copy_from(depth[i])
        layered.run(depth_buf, labels_buf, scale_factor)
        composite[i].copy_from(labels_buf.cu())
    scorer = LabelScorer(max(layered.num_layered_classes + 1, ds.num_classes()))
    return scorer.add(composite, truth, labels_reduce, per_image=True).result()


def _refit_on_dataset(forest, dataset_dir, num_images, min_count, fallback):
    """Refit `forest` (a DecisionForest) on `num_images` random images of a dataset directory (0: all of them); returns the
    LeafRefitter's report."""
    from .device import DeviceArray
    from .refit import LeafRefitter
    num_images = num_images or DecisionTreeDatasetConfig(dataset_dir).total_available_images
    ds = DecisionTreeDatasetConfig(dataset_dir, num_images=num_images, imgs_name='refit')
    assert ds.num_classes() <= int(forest.num_classes), "the dataset has classes the forest does not have"
    depth, labels = DeviceArray(ds.images_shape(), np.uint16), DeviceArray(ds.images_shape(), np.uint16)
    ds.get_depth_block_cu(0, depth)
    ds.get_labels_block_cu(0, labels)
    return LeafRefitter(forest).add(depth, labels).apply(min_count, fallback)


def refit_saved_model(model_path, dataset_dir, num_images, out_path, min_count=1, fallback='keep'):
    """Leaf refit of a saved forest (refit.LeafRefitter): the model's leaf PDFs re-estimated on `num_images` random images (0: all) of
    a dataset directory, read as score_saved_model reads them, and saved as the reference's .npy at `out_path`.  The tree
    structure is the model's own.  Returns the report of LeafRefitter.apply."""
    from .decision_tree import DecisionForest
    forest = DecisionForest.load(model_path)
    report = _refit_on_dataset(forest, dataset_dir, num_images, min_count, fallback)
    np.save(out_path, forest.forest_cu.get())
    return report


def fit_votes_saved_model(model_path, dataset_dir, num_images, out_path, min_count=8, max_var=DEFAULT_MAX_VAR, radius=255, chunk=64):
    """A joint-vote table for a saved forest (joint_votes.VoteFitter): `num_images` random images (0: all) of a dataset
    directory that carries joint targets (read_targets), read as score_saved_model reads them, summed `chunk` images a call,
    fitted with min_count and max_var (VoteFitter.fit's) and saved with VoteTable.save at `out_path`, which
    JointVoter takes through VoteTable.load.  Returns the fit's report."""
    from .decision_tree import DecisionForest
    from .device import DeviceArray
    from .joint_votes import VoteFitter
    forest = DecisionForest.load(model_path)
    num_images = num_images or DecisionTreeDatasetConfig(dataset_dir).total_available_images
    ds = DecisionTreeDatasetConfig(dataset_dir, num_images=num_images, imgs_name='votes')
    targets = read_targets(dataset_dir, ds.img_idxes)
    depth, labels = DeviceArray(ds.images_shape(), np.uint16), DeviceArray(ds.images_shape(), np.uint16)
    ds.get_depth_block_cu(0, depth)
    ds.get_labels_block_cu(0, labels)
    fitter = VoteFitter(forest, int(targets.shape[1]), radius=radius)
    for a in range(0, num_images, int(chunk)):
        fitter.add(depth[a:a + chunk], labels[a:a + chunk], targets[a:a + chunk])
    table = fitter.fit(min_count, max_var)
    table.save(out_path)
    return table.report


def _prune_on_dataset(forest, dataset_dir, num_images, cost_per_leaf, min_count, max_levels, truncate):
    """Prune `forest` (a DecisionForest) on `num_images` random images of a dataset directory (0: all of them); returns (the
    pruned forest -- `forest` itself, or with `truncate` the shallower one that is left --, the ForestPruner's report)."""
    from .device import DeviceArray
    from .prune import ForestPruner
    num_images = num_images or DecisionTreeDatasetConfig(dataset_dir).total_available_images
    ds = DecisionTreeDatasetConfig(dataset_dir, num_images=num_images, imgs_name='prune')
    assert ds.num_classes() <= int(forest.num_classes), "the dataset has classes the forest does not have"
    depth, labels = DeviceArray(ds.images_shape(), np.uint16), DeviceArray(ds.images_shape(), np.uint16)
    ds.get_depth_block_cu(0, depth)
    ds.get_labels_block_cu(0, labels)
    pruner = ForestPruner(forest).add(depth, labels)
    report = pruner.plan(cost_per_leaf, min_count, max_levels)
    pruner.apply()
    return (pruner.truncated() if truncate else forest), report


def prune_saved_model(model_path, dataset_dir, num_images, out_path, cost_per_leaf=0, min_count=0, max_levels=None, truncate=True):
    """Reduced-error pruning of a saved forest (prune.ForestPruner) on `num_images` random images (0: all) of a dataset directory
    -- frames the trainer has not seen --, read as score_saved_model reads them, and saved as the reference's .npy at `out_path`:
    with `truncate` at the depth that is left, which the loader infers from the shape, else at the model's own depth with
    records of zeros below the folded subtrees.  Returns the report of ForestPruner.plan."""
    from .decision_tree import DecisionForest
    forest = DecisionForest.load(model_path)
    pruned, report = _prune_on_dataset(forest, dataset_dir, num_images, cost_per_leaf, min_count, max_levels, truncate)
    np.save(out_path, pruned.forest_cu.get())
    return report


def train_forest(dataset_dir, num_train, num_test, proposals, proposals_block, out_trees, max_depth, out_path=None,
                 trees_to_try=None, train_block=None, log=print, tree_seed=None, group=None, device_score=False,
                 refit_dir=None, refit_images=0, refit_min_count=1, refit_fallback='keep',
                 prune_dir=None, prune_images=0, prune_cost=0, prune_min_count=0, prune_max_levels=None):
    """The flow of src/train_model.py:52-139 without its GLFW window: train `trees_to_try` candidate trees, keep
    the `out_trees` best by test accuracy, evaluate the forest, save it as the reference's .npy.

    tree_seed (not in the reference): candidate tree i draws its proposals from numpy.random.seed(tree_seed + i)
    instead of continuing the global stream.  That makes the candidates independent of each other, which is what
    lets them be trained on different GPUs: with torch.distributed initialised (one process per GPU), rank r trains
    candidates r, r + world, ...; the trees and their scores are exchanged with all_gather_object and every rank
    keeps the same best ones -- the same forest, bit for bit, as one process with the same tree_seed.

    device_score (not in the reference): score every candidate and the forest with score.LabelScorer on the device instead
    of reading the test set's label maps back for a numpy comparison; the truth is not copied to the host either.  The log
    lines, the selection, the return value and the saved file are the same.  The forest's Score (confusion matrix, per-class
    and per-image figures) is then kept as train_forest.last_score, None after a run without device_score.

    refit_dir (not in the reference): the finished forest's leaf PDFs are re-estimated on `refit_images` random images (0: all) of that
    dataset directory (refit.LeafRefitter, with refit_min_count and refit_fallback) before the forest is scored and saved:
    train on clean renders, refit on what the camera reports.  The candidates are selected as trained.  Without it nothing
    changes.

    prune_dir (not in the reference): after the optional refit and before the forest is scored and saved, it is pruned on
    `prune_images` random images (0: all) of that dataset directory -- frames the trainer has not seen -- by prune.ForestPruner
    with prune_cost a leaf, prune_min_count and prune_max_levels (its cost_per_leaf, min_count and max_levels), and cut to the
    depth D' that is left: the returned array and the saved .npy have depth D', which the loader infers from the shape, and the
    score is the pruned forest's.  The candidates are selected as trained.  Without it nothing changes."""
    from .decision_tree import DecisionForest, DecisionTree, DecisionTreeEvaluator, DecisionTreeTrainer
    from .device import DeviceArray
    from .util import MAX_UINT16
    trees_to_try = trees_to_try or out_trees
    if tree_seed is not None:
        np.random.seed(int(tree_seed))     # the random train/test split: the same in every process
    train_data, test_data = DecisionTreeDatasetConfig.multiple(dataset_dir, [(num_train, train_block, 'train'),
                                                                             (num_test, None, 'test')])
    trainer = DecisionTreeTrainer(train_block or num_train, proposals_block)
    evaluator = DecisionTreeEvaluator()
    tree1 = DecisionTree(max_depth, train_data.num_classes())
    trainer.allocate(train_data, proposals, tree1.max_depth)
    out_cu = DeviceArray(test_data.images_shape(), np.uint16)
    test_depth, test_labels = DeviceArray(test_data.images_shape(), np.uint16), DeviceArray(test_data.images_shape(), np.uint16)
    test_data.get_depth_block_cu(0, test_depth)
    test_data.get_labels_block_cu(0, test_labels)
    train_forest.last_score = None
    if device_score:
        from .score import LabelScorer
        scorer = LabelScorer(test_data.num_classes())
    else:
        truth = test_labels.get()
    best = [None] * out_trees
    forest_cpu = np.zeros((out_trees, tree1.TOTAL_TREE_NODES, tree1.TREE_NODE_ELS), dtype=np.float32)
    rank, world = 0, 1
    if tree_seed is not None:
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized():
            rank, world = dist.get_rank(group), dist.get_world_size(group)
    candidates = {}
    for i in range(rank, trees_to_try, world):
        if tree_seed is not None:
            np.random.seed(int(tree_seed) + i)
        trainer.train(train_data, tree1)
        out_cu.fill(MAX_UINT16)
        evaluator.get_labels(tree1, test_depth, out_cu)
        if device_score:
            pct = scorer.reset().add(out_cu, test_labels).result().pct_matching
        else:
            pct = float(np.sum(out_cu.get() == truth) / np.sum(truth > 0))
        log(f'tree {i}: pct. matching pixels: {pct:.4f}')
        candidates[i] = (pct, tree1.tree_out_cu.get())
    if world > 1:
        parts = [None] * world
        dist.all_gather_object(parts, candidates, group=group)
        candidates = {i: v for part in parts for i, v in part.items()}
    for i in range(trees_to_try):        # the reference's selection, in candidate order
        pct, tree_np = candidates[i]
        slot = -1
        if None in best:
            slot = best.index(None)
        elif pct > min(best):
            slot = best.index(min(best))
        if slot > -1:
            best[slot] = pct
            forest_cpu[slot] = tree_np
    forest = DecisionForest(out_trees, max_depth, test_data.num_classes())
    forest.forest_cu.set(forest_cpu)
    if refit_dir is not None:
        report = _refit_on_dataset(forest, refit_dir, refit_images, refit_min_count, refit_fallback)
        forest_cpu = forest.forest_cu.get()
        log(f'refit on {refit_images or "all"} images: {report["own"]} of {report["leaf_slots"]} leaf slots from their own counts, '
            f'{report["ancestor"]} from an ancestor, {report["kept"]} kept')
    if prune_dir is not None:
        forest, report = _prune_on_dataset(forest, prune_dir, prune_images, prune_cost, prune_min_count, prune_max_levels, True)
        forest_cpu = forest.forest_cu.get()
        log(f'pruned on {prune_images or "all"} images: {report["leaf_slots_before"]} -> {report["leaf_slots_after"]} leaf slots, '
            f'depth {report["depth"]}, errors of the trees alone {report["errors_before"]} -> {report["errors_after"]} of '
            f'{report["pixels"]} walks')
    out_cu.fill(MAX_UINT16)
    evaluator.get_labels_forest(forest, test_depth, out_cu)
    if device_score:
        train_forest.last_score = scorer.reset().add(out_cu, test_labels, per_image=True).result()
        pct = train_forest.last_score.pct_matching
    else:
        pct = float(np.sum(out_cu.get() == truth) / np.sum(truth > 0))
    log(f'FOREST pct. matching pixels: {pct:.4f}')
    if out_path:
        np.save(out_path, forest_cpu)
    return forest_cpu, pct


train_forest.last_score = None
