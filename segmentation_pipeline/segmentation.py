"""Drop-in ``segmentation_pipeline.segmentation``: same names as the reference module
(``/root/reference/segmentation_pipeline/segmentation.py``), backed by the MI355X-native HIP path.

    from segmentation_pipeline import segmentation
    cfg = segmentation.parse("config.yaml")      # reference :211-214
    cfg.fit(ds)                                   # reference README.md:125

What is mirrored: ``parse`` (sets ``cfg.path``), ``PipelineConfig`` with ``createNet`` / ``createNet1``
(the YAML -> constructor-kwargs rules of reference :96-155: ``activation: none``, architecture lookup
order, backbone check and its error messages, alias renaming, signature filtering, ``crops``),
``createStage`` / ``SegmentationStage.unfreeze`` (:49-50, :249-260), ``custom_models`` (:31-33), the
loss/metric name registry (:15-22), ``evaluate`` / ``update`` (:37-47, :58-60), ``predict_to_directory`` (:62-79) and
``load_writeable_dataset`` / ``create_writeable_dataset`` (:196-208).  The Keras / imgaug objects
behind those names are replaced by the HIP plan; nothing here computes on the CPU.
"""
import inspect
import os

import numpy as np

from segmentation_training_pipeline_amd import models as _models
from segmentation_training_pipeline_amd import pipeline as generic
from segmentation_training_pipeline_amd.pipeline import ALIASES, CUSTOM_KEYS

# name -> what the HIP loss/metric kernel provides (reference :15-22 registers these names with Keras)
custom_objects = {
    "dice": "dice", "iou": "iou", "iot": "iot", "dice_loss": "dice_loss", "binary_crossentropy": "binary_crossentropy",
    "categorical_crossentropy": "categorical_crossentropy", "binary_accuracy": "binary_accuracy",
    "iou_loss": "iou_loss", "jaccard_loss": "jaccard_loss", "focal_loss": "focal_loss",        # sigmoid head (stp_sigmoid_loss_ex)
    "lovasz_loss": "lovasz_loss",                                                                # sigmoid head (stp_lovasz_hinge)
    "lovasz_softmax": "lovasz_softmax",                                                          # softmax heads (stp_lovasz_softmax)
}
unsupported_objects = ()

extra_train = generic.extra_train     # name -> dataset added to every fold's training indexes (reference :29, README.md:698-709)
dataset_augmenters = {}

# name -> fn(**arch_kwargs) -> model; the reference ships one entry, its in-tree DeepLabV3+ (reference :31-33), and lets users
# add more (README.md:636-643)
custom_models = {"DeepLabV3": _models.Deeplabv3}


def ansemblePredictions(sourceFolder, folders, cb, data, weights=None):
    """Averages per-image .npy predictions of several folders (README.md:745-754)."""
    for f in sorted(os.listdir(sourceFolder)):
        stem = f[0:f.index(".")] if "." in f else f
        arrs = [np.load(os.path.join(d, stem + ".npy")) for d in folders]
        w = weights or [1.0] * len(arrs)
        cb(f, sum(a * wi for a, wi in zip(arrs, w)) / float(sum(w)), data)


def _impl(model):
    """The compiled HIP model behind what ``load_model`` returns (a models.SegModel), or the HipSegModel itself."""
    return model._need() if hasattr(model, "_need") else model


class SegmentationStage(generic.Stage):
    def unfreeze(self, model):
        # reference :259-260 -> segmentation_models.utils.set_trainable(model): every layer trainable
        model.freeze_encoder = False


class PipelineConfig(generic.GenericTaskConfig):
    def __init__(self, **atrs):
        super().__init__(**atrs)
        self.dataset_clazz = generic.KFoldedDataSet
        self.flipPred = True

    def createStage(self, x):
        return SegmentationStage(x, self)

    def evaluate(self, d, fold, stage, negatives="all", limit=16):
        """Reference :37-47: up to ``limit`` validation items of ``fold`` go through the validation pipeline
        (``transformAugmentor``: ``transforms`` + Resize, on the device) and ``model.predict``; yields the batch with
        ``images_aug`` and ``heatmaps_aug`` (one probability map per item, ``.arr`` H x W x classes) filled in."""
        mdl = self.load_model(fold, stage)
        ta = self.transformAugmentor()
        folds = self.kfold(d, range(0, len(d)))
        rs = folds.load(fold, False, negatives, limit)
        for z in ta.augment_batches([rs]):
            res = mdl.predict(np.array(z.images_aug))
            z.heatmaps_aug = [PredictedMap(x) for x in res]
            yield z

    def update(self, z, res):
        """Reference :58-60: attaches predictions ``res`` to the batch ``z`` as its ``segmentation_maps_aug``."""
        z.segmentation_maps_aug = [PredictedMap(x) for x in res]

    def _writeable(self, ds, path, count):
        from segmentation_pipeline.impl.datasets import CompressibleWriteableDS
        resName = (ds.name if hasattr(ds, "name") else "") + "_predictions"
        if self.compressScale is not None:
            return CompressibleWriteableDS(ds, resName, path, count, asUints=self.compressPredictionsAsInts, scale=self.compressScale)
        return CompressibleWriteableDS(ds, resName, path, count, asUints=self.compressPredictionsAsInts)

    def load_writeable_dataset(self, ds, path):
        """Reference :196-201: re-opens the predictions stored for ``ds`` under ``path`` (one entry per item of ``ds``)."""
        return self._writeable(ds, path, len(ds))

    def create_writeable_dataset(self, dataset, dsPath):
        """Reference :203-208: an empty predictions dataset over ``dataset`` stored under ``dsPath`` (``append`` + ``commit``)."""
        return self._writeable(dataset, dsPath, 0)

    def createNet(self):
        return self.createNet1(False)

    def createNet1(self, forInference):
        ac = self.all.get("activation")
        if ac == "none":
            ac = None
        self.all["activation"] = ac
        if self.architecture in custom_models:
            clazz = custom_models[self.architecture]
        else:
            if self.architecture not in _models.ARCHITECTURES:
                print("Unknown architecture:" + str(self.architecture))
                print("Known architectures:", sorted(_models.ARCHITECTURES))
                raise ValueError("Unknown architecture")
            clazz = _models.ARCHITECTURES[self.architecture]
            if str(self.backbone).lower() not in _models.known_backbones():
                print("Unknown backbone:" + str(self.backbone))
                print("Known backbones:", _models.known_backbones())
                raise ValueError("Unknown backbone")
        self.backbone = str(self.backbone).lower()
        self.all["backbone"] = self.backbone
        cleaned = {}
        sig = inspect.signature(clazz)
        for arg in self.all:
            pynama = ALIASES.get(arg, arg)
            if arg not in CUSTOM_KEYS and pynama in sig.parameters:
                cleaned[pynama] = self.all[arg]
        self.clean(cleaned)
        if forInference and "weights" in cleaned:
            cleaned["weights"] = None
        if forInference and "encoder_weights" in cleaned:
            cleaned["encoder_weights"] = None     # trained weights are loaded right after (load_model)
        if self.crops is not None and "input_shape" in cleaned:
            s = cleaned["input_shape"]
            cleaned["input_shape"] = (s[0] // self.crops, s[1] // self.crops, s[2])
        nchannel = None
        if "input_shape" in cleaned and cleaned["input_shape"][2] > 3:
            if cleaned["input_shape"][2] > 7:
                raise ValueError("the HIP backend takes images of up to 7 channels")
            # reference :135-153: with encoder_weights an N-channel model is built from the 3-channel pretrained one (adaptNet
            # copies the first convolution's kernels into the wider one, `copyWeights` seeds channel 3 from channel 2) and cached
            # as `<experiment>.mdl-nchannel`; without them the N-channel model is simply built.  The adaptation runs when the
            # model is compiled (models.adapt_nchannel), where the pretrained file is read.
            ew = cleaned.get("encoder_weights")
            if ew is not None and len(str(ew)) > 0:
                nchannel = {"cache": str(self.path) + ".mdl-nchannel", "copy": bool(self.all.get("copyWeights", False))}
        model = clazz(**cleaned)
        if nchannel is not None:
            model.nchannel_adapt = nchannel
        return model

    def load_model(self, fold=0, stage=-1):
        if self.windows is not None:
            self._check_windows()
        if stage < 0:
            stage = len(self.stages) + stage
        model = self.createNet1(True)
        st = self.stages[stage]
        model.compile(optimizer=self.optimizer, loss=(st.loss or self.loss), lr=self.lr, batch=self.inference_batch,
                      dtype=self.dtype)
        model.load_weights(self.weightsPath(fold, stage))
        return model

    def get_eval_batch(self):
        return self.inference_batch

    # ---------------------------------------------------------------- inference (reference :62-91, :158-191)
    def _models(self, fold, stage):
        folds = fold if isinstance(fold, (list, tuple)) else [fold]
        return [self.load_model(f, stage) for f in folds]

    def _resize_to_net(self, impl, images, device=False):
        """uint8 HxWxC images of any size -> uint8 [n, H, W, C] at the network shape (stp_augment_u8, identity + resize).
        ``device=True``: every image is resized into its slot of ONE device batch [impl.batch, H, W, C], which is returned as it is
        (the slots behind the n images are not written, and nothing reads them) - nothing comes back to the host."""
        from segmentation_training_pipeline_amd import ops
        import torch
        H, W, ch = impl.H, impl.W, impl.in_ch
        if device and len(images) > impl.batch:
            raise ValueError("%d images do not fit a batch of %d" % (len(images), impl.batch))
        xs = torch.empty((impl.batch if device else len(images), H, W, ch), dtype=torch.uint8, device=impl.device)
        for i, img in enumerate(images):
            img = np.asarray(img)
            if img.ndim == 2:
                img = img[:, :, None]
            if img.shape[2] < ch:
                if img.shape[2] != 1:
                    raise ValueError("image has %d channels, the network expects %d" % (img.shape[2], ch))
                img = np.repeat(img, ch, axis=2)
            img = np.ascontiguousarray(img[:, :, :ch], dtype=np.uint8)
            h, w = img.shape[:2]
            prm = torch.from_numpy(generic.augment.identity_batch(1, h, w, (H, W))).to(impl.device)
            src = torch.from_numpy(img).to(impl.device)
            ops.augment_u8(src, None, xs[i:i + 1], None, prm, 1, h, w, H, W, ch)
        return xs if device else xs.cpu().numpy()

    TTA_VALUES = "None / False (no augmentation), True (the two flips), 'd4' (the eight symmetries of the square)"

    @staticmethod
    def _tta_ops(ttflips):
        """The members of the square's symmetry group a ``ttflips`` value sums, in the order they are added: ``None`` / ``False``
        ``(0,)``, ``True`` (and any other non-string truthy value) ``(0, 1, 2)``, ``"d4"`` ``(0, ..., 7)``.  Member ``op`` is:
        transpose if ``op & 4``, then columns reversed if ``op & 1``, then rows reversed if ``op & 2`` (``_d4_apply``)."""
        if isinstance(ttflips, str):
            if ttflips != "d4":
                raise ValueError("ttflips %r: the accepted values are %s" % (ttflips, PipelineConfig.TTA_VALUES))
            return tuple(range(8))
        return (0, 1, 2) if ttflips else (0,)

    @staticmethod
    def _d4_apply(x, op):
        """Member ``op`` of the group on [n, H, W, C] (numpy view): whole pixels move, channels keep their order."""
        t = x.transpose(0, 2, 1, 3) if op & 4 else x
        t = t[:, :, ::-1] if op & 1 else t
        return t[:, ::-1] if op & 2 else t

    @staticmethod
    def _d4_invert(y, op):
        """The inverse of ``_d4_apply(., op)``: the same steps undone in reverse order."""
        u = y[:, ::-1] if op & 2 else y
        u = u[:, :, ::-1] if op & 1 else u
        return u.transpose(0, 2, 1, 3) if op & 4 else u

    def _check_tta(self, ttflips):
        """The ``ttflips`` value, checked before anything is loaded -> its ops.  ``"d4"`` holds transposing members: the network
        shape (after the ``crops`` division) has to be square."""
        ops_ = self._tta_ops(ttflips)
        if len(ops_) == 8:
            c = int(self.crops) if self.crops is not None else 1
            H, W = int(self.shape[0]) // c, int(self.shape[1]) // c
            self._d4_needs_square(H, W)
        return ops_

    @staticmethod
    def _d4_needs_square(H, W):
        if H != W:
            raise ValueError("ttflips='d4': the transposing members of the group need H == W and the network shape is %d x %d; "
                             "ttflips=True (the two flips) remains available" % (H, W))

    def predict_on_batch(self, models, ttflips, xs):
        """Mean of the fold models' probabilities, optionally with flip test-time augmentation (README.md:519-534) or, ``"d4"``, with
        all eight symmetries of the square (``_tta_ops``).  ``models``: one model or a list; ``xs``: uint8 [n, H, W, 3] at the network
        shape, n <= inference batch.
        Numpy in, numpy out: the host statement of what ``predict_on_batch_device`` + stp_predict_finish compute on the device."""
        models = models if isinstance(models, (list, tuple)) else [models]
        acc = np.zeros((len(xs),) + tuple(xs.shape[1:3]) + (self.classes,), np.float32)
        k = 0
        for m in models:
            for op in self._tta_ops(ttflips):
                acc += self._d4_invert(m.predict(self._d4_apply(xs, op)), op); k += 1
        return acc / k

    def predict_on_batch_device(self, models, ttflips, xs_dev, n):
        """``predict_on_batch`` without the host: ``xs_dev`` is a uint8 device tensor [batch, H, W, C] at the network shape whose first
        ``n`` images count.  Returns ``(acc, k)``: the float32 device SUM [batch, H, W, classes] of the k probability maps (models in
        order, each plain, then - ``ttflips`` - from the column-flipped and from the row-flipped input, un-flipped:
        stp_predict_accumulate; then - ``"d4"`` - from the other five members of the square's symmetry group, un-transformed:
        stp_predict_accumulate_dihedral) - the same additions in the same order as the host loop, so ``acc[:n] / k`` is its result
        bit for bit.
        ``acc`` is this config's one accumulator of that shape: it is zeroed and reused by the next call; stp_predict_finish turns an
        image's slice into the finished map."""
        for acc, k in self._sum_maps_device(models, ttflips, xs_dev, n):
            pass
        return acc, k

    def _sum_maps_device(self, models, ttflips, xs_dev, n):
        """The additions of ``predict_on_batch_device`` as a generator: yields ``(acc, k)`` after each of them (``find_tta`` reads
        the running sum on the way; stp_predict_finish does not modify it)."""
        from segmentation_training_pipeline_amd import ops
        import torch
        tta = self._tta_ops(ttflips)
        impls = [_impl(m) for m in (models if isinstance(models, (list, tuple)) else [models])]
        i0 = impls[0]
        if len(tta) == 8:
            self._d4_needs_square(i0.H, i0.W)
        key = (str(i0.device), i0.batch, i0.H, i0.W, int(self.classes))
        cache = self.__dict__.setdefault("_accumulators", {})
        numel = int(np.prod(key[1:]))
        if key not in cache:          # (stp_zero_bytes clears whole 16-byte words: the buffer is rounded up to them)
            cache[key] = torch.empty(-(-numel // 4) * 4, dtype=torch.float32, device=i0.device)
        ops.zero_bytes(cache[key], cache[key].numel() * 4)
        acc = cache[key][:numel].view(key[1:])
        k = 0
        for impl in impls:
            for flip in tta:
                probs = impl.predict_device(xs_dev, n, flip)
                if flip < 3:
                    ops.predict_accumulate(probs, acc, int(n), i0.H, i0.W, int(self.classes), flip)
                else:
                    ops.predict_accumulate_dihedral(probs, acc, int(n), i0.H, i0.W, int(self.classes), flip)
                k += 1
                yield acc, k

    @staticmethod
    def _scale_back(p, h, w):
        """Prediction at the network shape -> original image size (nearest, like the reference's Scale of a map)."""
        yy = (np.arange(h) * p.shape[0] // h)[:, None]
        xx = (np.arange(w) * p.shape[1] // w)[None, :]
        return p[yy, xx]

    # what stp_predict_finish writes: float32 H x W x classes probabilities, their `* 255` bytes, or the uint8 H x W label map
    PROBS, BYTES, LABELS = 0, 1, 2

    @staticmethod
    def _new_map(acc, mode, h, w):
        import torch
        shape = (h, w) if mode == PipelineConfig.LABELS else (h, w, acc.shape[-1])
        return torch.empty(shape, dtype=torch.float32 if mode == PipelineConfig.PROBS else torch.uint8, device=acc.device)

    def _predict_maps_device(self, models, ttflips, items, mode=0, original_size=True):
        """``_predict_maps`` without the copy back: ``(maps, whole)`` - one DEVICE tensor per item (``mode``: PROBS / BYTES / LABELS, at
        the item's own size or, ``original_size=False`` and no ``crops``, at the network shape), and, where the items share a size, the
        one tensor [n * h, w, ...] whose row blocks they are (else None).  The mask methods go on from here on the device."""
        from segmentation_training_pipeline_amd import ops
        if self.windows is not None:
            return [self._predict_windows_device(models, ttflips, it.x, mode) for it in items], None
        if self.crops:
            return [self._predict_cells_device(models, ttflips, it.x, mode) for it in items], None
        impl0 = _impl(models[0])
        H, W = impl0.H, impl0.W
        acc, k = self.predict_on_batch_device(models, ttflips, self._resize_to_net(impl0, [it.x for it in items], device=True), len(items))
        sizes = [tuple(it.x.shape[:2]) if original_size else (H, W) for it in items]
        if len(set(sizes)) == 1:
            h, w = sizes[0]
            out = self._new_map(acc, mode, len(items) * h, w)
            for i in range(len(items)):
                ops.predict_finish(acc[i], H, W, acc.shape[-1], k, mode, out[i * h:(i + 1) * h], h, w)
            return [out[i * h:(i + 1) * h] for i in range(len(items))], out
        maps = []
        for i, (h, w) in enumerate(sizes):
            out = self._new_map(acc, mode, h, w)
            ops.predict_finish(acc[i], H, W, acc.shape[-1], k, mode, out, h, w)
            maps.append(out)
        return maps, None

    def _predict_maps(self, models, ttflips, items, mode=0, original_size=True):
        """The finished maps (numpy, ``mode``: PROBS / BYTES / LABELS) of up to one batch of items, at each item's own size (or, with
        ``original_size=False`` and no ``crops``, at the network shape).  Resize, flips, the sum over models and flips, the mean, the
        way back to the image's size and the quantisation all run on the device; the finished maps of a batch come back in one copy
        when they share a size, one copy per item otherwise."""
        if self.windows is not None:
            return [self._predict_windows(models, ttflips, it.x, mode) for it in items]
        if self.crops:
            return [self._predict_cells(models, ttflips, it.x, mode) for it in items]
        maps, whole = self._predict_maps_device(models, ttflips, items, mode, original_size)
        if whole is not None:
            return list(whole.cpu().numpy().reshape((len(items), whole.shape[0] // len(items)) + tuple(whole.shape[1:])))
        return [m.cpu().numpy() for m in maps]

    def _predict_batches(self, spath, fold, stage, limit, ttflips, mode=0, original_size=True, device=False):
        from segmentation_pipeline.impl.datasets import DirectoryDataSet
        if self.windows is not None:
            self._check_windows()
        self._check_tta(ttflips)
        nets_ = self._models(fold, stage)
        ds = DirectoryDataSet(spath)
        n = len(ds) if limit < 0 else min(limit, len(ds))
        B = nets_[0].impl.batch
        for s in range(0, n, B):
            items = [ds[i] for i in range(s, min(s + B, n))]
            if device:
                yield items, self._predict_maps_device(nets_, ttflips, items, mode, original_size)[0]
            else:
                yield items, self._predict_maps(nets_, ttflips, items, mode, original_size)

    def predict_on_directory(self, spath, fold=0, stage=0, limit=-1, batch_size=32, ttflips=False):
        """Yields (items, probabilities) per batch: a float32 array [n, H, W, classes] at the network shape, or - ``crops`` or
        ``windows`` - the list of the items' assembled maps at their own sizes."""
        for items, maps in self._predict_batches(spath, fold, stage, limit, ttflips, self.PROBS, original_size=False):
            yield items, (maps if self.crops or self.windows is not None else np.stack(maps))

    def _predict_cells(self, models, ttflips, img, mode=0):
        """``crops: N`` at prediction time (README.md:488-491): the image is split into the N x N cells the model was trained
        on, every cell is predicted, scaled back to its own size and the map is assembled - invisible to the caller.  Each cell is
        finished into its rectangle of the full-size device map (stp_predict_finish with the map's row pitch); one copy brings it back."""
        return self._predict_cells_device(models, ttflips, img, mode).cpu().numpy()

    def _predict_cells_device(self, models, ttflips, img, mode=0):
        """The assembled full-size map of ``_predict_cells``, left on the device."""
        from segmentation_training_pipeline_amd import ops
        from segmentation_training_pipeline_amd.pipeline import crop_bounds
        c = int(self.crops)
        h, w = img.shape[:2]
        ys, xs_ = crop_bounds(h, c), crop_bounds(w, c)
        cells = [img[ys[r]:ys[r + 1], xs_[q]:xs_[q + 1]] for r in range(c) for q in range(c)]
        impl0 = _impl(models[0])
        out = None
        for s in range(0, len(cells), impl0.batch):
            chunk = cells[s:s + impl0.batch]
            acc, k = self.predict_on_batch_device(models, ttflips, self._resize_to_net(impl0, chunk, device=True), len(chunk))
            if out is None:
                out = self._new_map(acc, mode, h, w)      # (the cells tile it: every pixel is written)
            for j, cell in enumerate(chunk):
                r, q = divmod(s + j, c)
                ops.predict_finish(acc[j], impl0.H, impl0.W, acc.shape[-1], k, mode, out[ys[r]:ys[r + 1], xs_[q]:xs_[q + 1]],
                                   cell.shape[0], cell.shape[1], out_ld=w)
        return out

    # ---------------------------------------------------------------- sliding windows (csrc/window.hip; `windows: <overlap>`)
    @staticmethod
    def window_origins(size, L, overlap):
        """Origins of the windows of length ``L`` along one axis of ``size`` pixels: stride ``L - overlap``, the last window shifted
        back so that it ends at the image's edge; ``[0]`` where one window holds the axis."""
        size, L, overlap = int(size), int(L), int(overlap)
        if size <= L:
            return [0]
        return list(range(0, size - L, L - overlap)) + [size - L]

    @staticmethod
    def window_ramp(L, overlap):
        """int64 [L]: the cross-fade weight ``min(i + 1, L - i, overlap + 1)`` of a window's pixel i along one axis."""
        i = np.arange(int(L), dtype=np.int64)
        return np.minimum(np.minimum(i + 1, int(L) - i), int(overlap) + 1)

    @staticmethod
    def window_sums(size, L, overlap):
        """int64 [size]: per pixel of one axis, the sum of the ramps of the windows that hold it.  The windows of an image form a
        product grid and a window's weight is ``ramp_y * ramp_x``, so the weight sum of pixel (y, x) is ``sy[y] * sx[x]``."""
        ramp = PipelineConfig.window_ramp(L, overlap)
        sums = np.zeros(int(size), np.int64)
        for o in PipelineConfig.window_origins(size, L, overlap):
            n = min(int(L), int(size) - o)
            sums[o:o + n] += ramp[:n]
        return sums

    WINDOW_WEIGHT_LIMIT = 2 ** 24      # k * sy * sx stays an exact float32 integer

    def _check_windows(self, k=None, size=None):
        """The ``windows`` key, checked before anything is loaded: an integer overlap of at most half the network shape, not
        together with ``crops``; with ``k`` (maps summed per window) and an image ``size``: every denominator ``k * sy[y] * sx[x]``
        is an integer that float32 holds exactly."""
        v = self.windows
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError("windows: the overlap of neighbouring windows in pixels, an integer: got %r" % (v,))
        H, W = int(self.shape[0]), int(self.shape[1])
        if not 0 <= v <= min(H, W) // 2:
            raise ValueError("windows: %d is outside 0..%d (half the network shape %d x %d)" % (v, min(H, W) // 2, H, W))
        if self.crops is not None:
            raise ValueError("windows and crops are two ways to predict a large image: set one (windows: %r, crops: %r)" % (v, self.crops))
        if k is not None:
            top = int(k) * int(self.window_sums(size[0], H, v).max()) * int(self.window_sums(size[1], W, v).max())
            if top > self.WINDOW_WEIGHT_LIMIT:
                raise ValueError("windows: %d with %d maps per window gives a weight sum of %d, above 2**24: float32 would round it"
                                 % (v, k, top))

    def _predict_windows(self, models, ttflips, img, mode=0):
        """``windows: <overlap>`` at prediction time: the image is predicted at its own pixel scale in overlapping windows of the
        network shape, cross-faded where they overlap - no resize, no seams.  All of it runs on the device; one copy brings the
        finished map (``mode``: PROBS / BYTES / LABELS, at the image's size) back."""
        return self._predict_windows_device(models, ttflips, img, mode).cpu().numpy()

    def _predict_windows_device(self, models, ttflips, img, mode=0):
        """The finished map of ``_predict_windows``, left on the device.  The image goes to the device once; its windows are taken in
        raster order in chunks of the inference batch: stp_window_gather_u8 cuts a chunk into a batch at the network shape,
        ``predict_on_batch_device`` sums the fold models' (and flips') probabilities, stp_window_accumulate adds the ramp-weighted
        sums into the full-size canvas in window order; stp_window_finish divides by the weight sum."""
        from segmentation_training_pipeline_amd import ops
        import torch
        models = models if isinstance(models, (list, tuple)) else [models]
        impl0 = _impl(models[0])
        H, W, ch = impl0.H, impl0.W, impl0.in_ch
        img = np.asarray(img)
        if img.ndim == 2:
            img = img[:, :, None]
        if img.shape[2] < ch:      # (the channels as _resize_to_net prepares them: grey repeated, extra bands cut)
            if img.shape[2] != 1:
                raise ValueError("image has %d channels, the network expects %d" % (img.shape[2], ch))
            img = np.repeat(img, ch, axis=2)
        img = np.ascontiguousarray(img[:, :, :ch], dtype=np.uint8)
        h, w = img.shape[:2]
        self._check_windows(len(models) * len(self._tta_ops(ttflips)), (h, w))
        ov, classes = int(self.windows), int(self.classes)
        origins = [(y0, x0) for y0 in self.window_origins(h, H, ov) for x0 in self.window_origins(w, W, ov)]
        dev = impl0.device
        src = torch.from_numpy(img).to(dev)
        sy = torch.from_numpy(self.window_sums(h, H, ov).astype(np.float32)).to(dev)
        sx = torch.from_numpy(self.window_sums(w, W, ov).astype(np.float32)).to(dev)
        xs = torch.empty((impl0.batch, H, W, ch), dtype=torch.uint8, device=dev)
        numel = h * w * classes
        canvas = torch.empty(-(-numel // 4) * 4, dtype=torch.float32, device=dev)      # (stp_zero_bytes clears whole 16-byte words)
        ops.zero_bytes(canvas, canvas.numel() * 4)
        k = 0
        for s in range(0, len(origins), impl0.batch):
            chunk = origins[s:s + impl0.batch]
            ops.window_gather_u8(src, h, w, ch, chunk, xs, H, W)
            acc, k = self.predict_on_batch_device(models, ttflips, xs, len(chunk))
            ops.window_accumulate(acc, H, W, classes, chunk, ov, canvas, h, w)
        out = self._new_map(acc, mode, h, w)
        ops.window_finish(canvas, h, w, classes, k, sy, sx, mode, out)
        return out

    def predict_to_directory(self, spath, tpath, fold=0, stage=0, limit=-1, batchSize=32, binaryArray=False, ttflips=False, labelMap=False):
        """Writes one prediction per image of ``spath`` into ``tpath``: ``<stem>.png`` = probability of channel 0 as bytes (a
        multi-label head: ``<stem>_<c>.png`` per class), ``binaryArray``: ``<stem>.npy`` = float32 H x W x classes.
        ``labelMap=True``: ``<stem>.png`` holds the class index per pixel - the first largest of a softmax head's averaged
        probabilities, 0/1 (probability > 0.5) for a one-class head; a multi-label head has no single label per pixel (ValueError)."""
        multilabel = self.classes > 1 and self.all.get("activation") == "sigmoid"      # (independent sigmoid maps, H x W x classes)
        if labelMap and multilabel:
            raise ValueError("labelMap needs one label per pixel: a multi-label sigmoid head (classes: %d, activation: sigmoid) has "
                             "independent maps - write them with labelMap=False" % self.classes)
        if labelMap and binaryArray:
            raise ValueError("labelMap writes PNGs of class indices, binaryArray writes float32 arrays: choose one")
        if self.windows is not None:
            self._check_windows()
        self._check_tta(ttflips)
        os.makedirs(tpath, exist_ok=True)
        from PIL import Image
        mode = self.LABELS if labelMap else (self.PROBS if binaryArray else self.BYTES)
        for items, maps in self._predict_batches(spath, fold, stage, limit, ttflips, mode):
            for it, m in zip(items, maps):
                stem = it.id[0:it.id.index(".")] if "." in it.id else it.id
                if binaryArray:
                    np.save(os.path.join(tpath, stem), m)
                elif labelMap:
                    Image.fromarray(m).save(os.path.join(tpath, stem + ".png"))
                elif multilabel:              # one PNG per class: <stem>_<c>.png
                    for c in range(m.shape[2]):
                        Image.fromarray(np.ascontiguousarray(m[:, :, c])).save(os.path.join(tpath, "%s_%d.png" % (stem, c)))
                else:
                    Image.fromarray(np.ascontiguousarray(m[:, :, 0])).save(os.path.join(tpath, stem + ".png"))

    def predict_in_directory(self, spath, fold, stage, cb=None, data=None, limit=-1, batchSize=32, ttflips=False):
        """Calls ``cb(file_name, map, data)`` per image with ``map.arr`` = probabilities at the ORIGINAL image size
        (reference :81-91; README.md:498-527).  ``fold`` may be a list (ensemble).  The README's ensembling example
        omits ``stage`` (``predict_in_directory(path, folds, cb, data)``): that call shape is accepted too."""
        if callable(stage):
            stage, cb, data = 0, stage, cb
        for items, maps in self._predict_batches(spath, fold, stage, limit, ttflips):
            for it, m in zip(items, maps):
                cb(it.id, PredictedMap(m), data)

    def evaluateAll(self, ds, fold, stage=-1, negatives="real", ttflips=None):
        """Iterator over validation batches of ``fold`` (reference :158-191): each carries the original ``images``,
        ``data`` (ids), ``segmentation_maps`` (ground truth) and ``predicted_maps_aug`` (probabilities, original size)."""
        self._check_tta(ttflips)
        folds = self.kfold(ds, range(0, len(ds)))
        indexes = [int(i) for i in folds.sampledIndexes(fold, False, negatives)]
        m = self.load_model(fold, stage)
        B = m.impl.batch
        for s in range(0, len(indexes), B):
            items = [ds[i] for i in indexes[s:s + B]]
            maps = self._predict_maps([m], ttflips, items)
            yield EvalBatch(images=[it.x for it in items], data=[it.id for it in items],
                            segmentation_maps=[PredictedMap(np.asarray(it.y)) for it in items],
                            predicted_maps_aug=[PredictedMap(p) for p in maps])

    # ---------------------------------------------------------------- masks on the device (csrc/mask.hip; README.md:498-525, :541-550)
    SWEEP_METRICS = ("dice", "iou", "f2")

    def _softmax_head(self):
        return self.classes > 1 and self.all.get("activation") != "sigmoid"

    def _mask_mode(self, threshold, opening, closing, channel, min_size=0, area_threshold=0):
        """stp_mask_threshold's mode for this head (0: sigmoid map > threshold, 1: softmax argmax == channel), after the argument checks
        every mask method makes before a model is loaded."""
        if self.windows is not None:
            self._check_windows()
        if not 0 <= int(channel) < int(self.classes):
            raise ValueError("channel %r: the head has %d class(es)" % (channel, self.classes))
        for name, r in (("opening", opening), ("closing", closing)):
            if int(r) != r or not 0 <= r <= 7:
                raise ValueError("%s is the radius of a disk, 0 (off) to 7: got %r" % (name, r))
        for name, v in (("min_size", min_size), ("area_threshold", area_threshold)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 0:
                raise ValueError("%s is a pixel count, an integer >= 0 (0: off): got %r" % (name, v))
        if self._softmax_head():
            if threshold != 0.5:
                raise ValueError("a softmax head has one label per pixel: the mask of `channel` is argmax == channel and takes no threshold")
            return 1
        return 0

    def _device_mask(self, probs, mode, threshold, opening, closing, channel, min_size=0, area_threshold=0):
        """One image's finished device map [h, w, classes] -> its uint8 {0, 1} device mask [h, w]: stp_mask_threshold, then the disk
        opening (erode, dilate), then the disk closing (dilate, erode) - scipy.ndimage's binary_opening / binary_closing with defaults -,
        then stp_mask_area_filter in place: skimage's remove_small_objects(min_size), remove_small_holes(area_threshold), connectivity
        1.  A step whose argument is 0 launches nothing."""
        from segmentation_training_pipeline_amd import ops
        import torch
        h, w, C = (int(v) for v in probs.shape)
        a = torch.empty((h, w), dtype=torch.uint8, device=probs.device)
        ops.mask_threshold(probs, h, w, C, channel, mode, threshold, a)
        if opening or closing:
            b = torch.empty_like(a)
            for r, first in ((opening, 0), (closing, 1)):
                if r:
                    ops.mask_morph(a, b, h, w, r, first)
                    ops.mask_morph(b, a, h, w, r, 1 - first)
        if min_size or area_threshold:
            ws = torch.empty(ops.mask_area_filter_workspace_bytes(h, w), dtype=torch.uint8, device=probs.device)
            for size, invert in ((min_size, 0), (area_threshold, 1)):
                if size:
                    ops.mask_area_filter(a, a, h, w, 1, invert, size, ws)
        return a

    @staticmethod
    def _device_rle(mask):
        """The reference's run-length string (impl.rle.rle_encode) of a device mask: stp_mask_rle, then the count and the first
        ``count`` (start, length) pairs come back."""
        from segmentation_training_pipeline_amd import ops
        import torch
        h, w = (int(v) for v in mask.shape)
        runs = torch.empty(((h * w + 1) // 2, 2), dtype=torch.int32, device=mask.device)
        count = torch.empty(1, dtype=torch.int32, device=mask.device)
        ws = torch.empty(ops.mask_rle_workspace_bytes(h, w), dtype=torch.uint8, device=mask.device)
        ops.mask_rle(mask, h, w, runs, count, ws)
        n = int(count.item())
        return " ".join(map(str, runs[:n].reshape(-1).cpu().numpy().tolist()))      # "start length start length ..."

    @staticmethod
    def _device_labels(mask):
        """-> (int32 device label image [h, w], count): the 8-connected components of a device mask in scipy's / skimage's numbering
        (stp_mask_label, connectivity 2)."""
        from segmentation_training_pipeline_amd import ops
        import torch
        h, w = (int(v) for v in mask.shape)
        labels = torch.empty((h, w), dtype=torch.int32, device=mask.device)
        count = torch.empty(1, dtype=torch.int32, device=mask.device)
        ws = torch.empty(ops.mask_label_workspace_bytes(h, w), dtype=torch.uint8, device=mask.device)
        ops.mask_label(mask, h, w, 2, 0, labels, count, ws)
        return labels, count

    @staticmethod
    def _group_runs(runs, count):
        """(value, start, length) triples in ascending start -> one ``"start length ..."`` string per value 1..count: a stable sort by
        value keeps each value's runs in order."""
        runs = np.asarray(runs).reshape(-1, 3)
        runs = runs[np.argsort(runs[:, 0], kind="stable")]
        cuts = np.searchsorted(runs[:, 0], np.arange(1, count + 2))
        return [" ".join(map(str, runs[cuts[k]:cuts[k + 1], 1:].reshape(-1).tolist())) for k in range(count)]

    @classmethod
    def _device_label_codes(cls, labels, count):
        """One run-length string per value 1..count of a device label image: stp_label_rle, then the two counts and the first ``runs``
        triples come back and are grouped by label on the host."""
        from segmentation_training_pipeline_amd import ops
        import torch
        h, w = (int(v) for v in labels.shape)
        runs = torch.empty((h * w, 3), dtype=torch.int32, device=labels.device)
        nruns = torch.empty(1, dtype=torch.int32, device=labels.device)
        ws = torch.empty(ops.label_rle_workspace_bytes(h, w), dtype=torch.uint8, device=labels.device)
        ops.label_rle(labels, h, w, runs, nruns, ws)
        n, k = int(count.item()), int(nruns.item())
        return cls._group_runs(runs[:k].cpu().numpy(), n)

    @classmethod
    def _device_multi_rle(cls, mask):
        """impl.rle.multi_rle_encode of a device mask: stp_mask_label (connectivity 2), then ``_device_label_codes``."""
        return cls._device_label_codes(*cls._device_labels(mask))

    def predict_masks(self, spath, fold=0, stage=0, limit=-1, ttflips=False, threshold=0.5, opening=0, closing=0, channel=0, rle=True):
        """README.md:498-525 without the host: a generator of ``(file_name, rle_string)`` - or, ``rle=False``, ``(file_name, uint8 h x w
        mask)`` - per image of ``spath``.  Per image, on the device: the finished map at the image's own size (``fold`` may be a list,
        ``ttflips`` and ``crops:`` as in ``predict_in_directory``), ``map[..., channel] > float32(threshold)`` (a softmax head: ``argmax
        == channel``, no threshold), a disk(``opening``) opening, a disk(``closing``) closing (radius 0: off; both as
        scipy.ndimage's binary_opening / binary_closing with defaults - that closing clears a band at the image border), the
        run-length code.  Only the runs (or the mask) come back.  Connected-component clean-up and per-object codes
        (remove_small_objects, remove_small_holes, multi_rle_encode) are ``predict_masks_ex``: this method with three more keywords."""
        return self.predict_masks_ex(spath, fold, stage, limit, ttflips, threshold, opening, closing, channel, rle)

    def predict_masks_ex(self, spath, fold=0, stage=0, limit=-1, ttflips=False, threshold=0.5, opening=0, closing=0, channel=0, rle=True,
                         min_size=0, area_threshold=0, components=False):
        """``predict_masks`` (same arguments, same launches when the three new keywords keep their defaults) with the README's
        connected-component steps on the device: after the closing, skimage's ``remove_small_objects(mask, min_size)`` and then
        ``remove_small_holes(mask, area_threshold)`` (integers >= 0, 0: off; connectivity 1, skimage's default; README.md:498-525
        uses 64 and 64), then the run-length code.  ``components=True`` splits the final mask into its 8-connected objects:
        ``(file_name, [rle_string, ...])``, one string per object in label order - exactly
        ``impl.rle.multi_rle_encode(mask[:, :, None])``, ``[]`` for an empty mask - or, ``rle=False``, ``(file_name, int32 h x w label
        image)`` in scipy.ndimage.label's numbering.  Only the runs (or the mask, or the labels) come back."""
        mode = self._mask_mode(threshold, opening, closing, channel, min_size, area_threshold)      # (refusals fire here, not at the first next())
        self._check_tta(ttflips)

        def masks():
            for items, maps in self._predict_batches(spath, fold, stage, limit, ttflips, self.PROBS, device=True):
                for it, probs in zip(items, maps):
                    mask = self._device_mask(probs, mode, float(threshold), int(opening), int(closing), int(channel), int(min_size),
                                             int(area_threshold))
                    if components:
                        yield it.id, (self._device_multi_rle(mask) if rle else self._device_labels(mask)[0].cpu().numpy())
                    else:
                        yield it.id, (self._device_rle(mask) if rle else mask.cpu().numpy())
        return masks()

    def predict_to_csv(self, spath, csv_path, fold=0, stage=0, limit=-1, ttflips=False, threshold=0.5, opening=0, closing=0, channel=0,
                       columns=("image", "rle_mask"), min_size=0, area_threshold=0, components=False):
        """README.md:498-525 in one call: ``predict_masks_ex`` written as a CSV with the header ``columns``; the image column holds the file
        name up to its first ``.``.  ``components=True``: one row per object, the image name repeated; an image without objects gets
        one row with an empty code.  Returns the number of rows."""
        if len(columns) != 2:
            raise ValueError("columns names the image column and the run-length column")
        rows = self.predict_masks_ex(spath, fold, stage, limit, ttflips, threshold, opening, closing, channel, True, min_size, area_threshold,
                                     components)
        return self._write_csv(csv_path, columns, rows, components)

    @staticmethod
    def _write_csv(csv_path, columns, rows, per_object):
        """The CSV of ``predict_to_csv`` / ``predict_instances_to_csv``: the header ``columns``, then per ``(name, code)`` of ``rows`` one row
        - ``per_object``: one row per string of the list ``code``, and one row with an empty code for an empty list.  Returns the number of
        rows."""
        import csv
        n = 0
        with open(csv_path, "w", newline="") as f:
            out = csv.writer(f, lineterminator="\n")
            out.writerow(list(columns))
            for name, code in rows:
                for c in ((code or [""]) if per_object else [code]):
                    out.writerow([name[0:name.index(".")] if "." in name else name, c])
                    n += 1
        return n

    @staticmethod
    def sweep_score(metric, P, TP, G):
        """float64 scores from integer counters (arrays broadcast): P predicted, TP true positive, G positives of the target.
        dice 2TP / (P + G), iou TP / (P + G - TP), f2 5TP / (4G + P); 1 where P = G = 0."""
        P, TP, G = (np.asarray(a, np.float64) for a in (P, TP, G))
        num, den = {"dice": (2 * TP, P + G), "iou": (TP, P + G - TP), "f2": (5 * TP, 4 * G + P)}[metric]
        empty = (P == 0) & (G == 0)
        return np.where(empty, 1.0, num / np.where(empty, 1.0, den))

    def find_threshold(self, ds, fold, stage=-1, negatives="real", ttflips=None, thresholds=None, metric="dice", average="image", channel=0):
        """README.md:541-550 without the host passes: the threshold (of ``thresholds``, default d / 20 for d = 1..19) whose masks
        ``map[..., channel] > threshold`` score best against the validation masks of ``fold`` (the items ``evaluateAll`` yields).  Each
        image makes ONE stp_threshold_counts pass on the device; only the integer counters come back, and the scores are float64 on
        the host: ``average="image"`` the mean of the per-image scores, ``"pixels"`` the score of the summed counters.  Returns
        ``(best_threshold, {threshold: score})``; the first threshold wins a tie.  No opening inside the sweep."""
        from segmentation_training_pipeline_amd import ops
        import torch
        if self._softmax_head():
            raise ValueError("find_threshold sweeps the threshold of a sigmoid map: a softmax head has none")
        if metric not in self.SWEEP_METRICS:
            raise ValueError("metric %r: one of %s" % (metric, ", ".join(self.SWEEP_METRICS)))
        if average not in ("image", "pixels"):
            raise ValueError("average %r: 'image' or 'pixels'" % (average,))
        if not 0 <= int(channel) < int(self.classes):
            raise ValueError("channel %r: the head has %d class(es)" % (channel, self.classes))
        self._check_tta(ttflips)
        thresholds = [d / 20 for d in range(1, 20)] if thresholds is None else [float(t) for t in thresholds]
        t32 = np.asarray(thresholds, np.float32)            # what the device compares with
        if not 1 <= len(thresholds) <= 64:
            raise ValueError("1 to 64 thresholds in one sweep: got %d" % len(thresholds))
        if not np.isfinite(t32).all() or not (np.diff(t32) > 0).all():
            raise ValueError("thresholds must be finite and strictly ascending (as float32)")
        folds = self.kfold(ds, range(0, len(ds)))
        indexes = [int(i) for i in folds.sampledIndexes(fold, False, negatives)]
        if not indexes:
            raise ValueError("fold %r has no validation items" % (fold,))
        m = self.load_model(fold, stage)
        dev, B, T = m.impl.device, m.impl.batch, len(thresholds)
        counts = torch.empty((len(indexes), T, 2), dtype=torch.int64, device=dev)
        totals = torch.empty((len(indexes), 2), dtype=torch.int64, device=dev)
        ws = torch.empty(ops.threshold_counts_workspace_bytes(T), dtype=torch.uint8, device=dev)
        for s in range(0, len(indexes), B):
            items = [ds[i] for i in indexes[s:s + B]]
            for j, (it, probs) in enumerate(zip(items, self._predict_maps_device([m], ttflips, items)[0])):
                y = np.asarray(it.y)
                plane = y if y.ndim == 2 else y[:, :, channel if y.shape[2] > 1 else 0]
                h, w, C = (int(v) for v in probs.shape)
                if plane.shape != (h, w):
                    raise ValueError("item %r: a %s mask for a %d x %d image" % (it.id, plane.shape, h, w))
                target = torch.from_numpy(np.ascontiguousarray(plane != 0).view(np.uint8)).to(dev)
                ops.threshold_counts(probs, target, h, w, C, channel, t32, counts[s + j], totals[s + j], ws)
        counts, totals = counts.cpu().numpy(), totals.cpu().numpy()          # the only copies back: 2 T + 2 integers per image
        if average == "pixels":
            scores = self.sweep_score(metric, counts[:, :, 0].sum(0), counts[:, :, 1].sum(0), totals[:, 0].sum())
        else:
            scores = self.sweep_score(metric, counts[:, :, 0], counts[:, :, 1], totals[:, :1]).mean(axis=0)
        table = {t: float(v) for t, v in zip(thresholds, scores)}
        return thresholds[int(np.argmax(scores))], table

    def find_tta(self, ds, fold, stage=-1, negatives="real", threshold=0.5, metric="dice", average="image", channel=0):
        """Whether test-time augmentation pays for this model: the ``find_threshold`` score (same items, formulas, ``metric`` and
        ``average``) of the masks ``map[..., channel] > threshold`` predicted with ``ttflips`` = ``False``, ``True`` and ``"d4"``.  The
        eight passes run ONCE per batch; the running sum is read after member 1 (k = 1), member 3 (k = 3) and member 8 (k = 8) - each
        read is stp_predict_finish to the image's size (it leaves the accumulator as it is) and one stp_threshold_counts - so every
        entry equals ``find_threshold(..., ttflips=v, thresholds=[threshold])[1][threshold]`` exactly.  Returns ``(best, {False:
        score, True: score, "d4": score})``; the first of ``False, True, "d4"`` wins a tie.  One fold; no ``windows`` / ``crops``."""
        from segmentation_training_pipeline_amd import ops
        import torch
        if self._softmax_head():
            raise ValueError("find_tta scores thresholded sigmoid maps, as find_threshold: a softmax head has no threshold")
        if metric not in self.SWEEP_METRICS:
            raise ValueError("metric %r: one of %s" % (metric, ", ".join(self.SWEEP_METRICS)))
        if average not in ("image", "pixels"):
            raise ValueError("average %r: 'image' or 'pixels'" % (average,))
        if not 0 <= int(channel) < int(self.classes):
            raise ValueError("channel %r: the head has %d class(es)" % (channel, self.classes))
        if isinstance(fold, (list, tuple)):
            raise ValueError("find_tta takes one fold, as find_threshold: got %r" % (fold,))
        if self.windows is not None or self.crops:
            raise ValueError("find_tta does not cover `windows` / `crops` configurations yet: compare find_threshold(ttflips=...) calls")
        self._check_tta("d4")
        t32 = np.asarray([float(threshold)], np.float32)            # what the device compares with
        if not np.isfinite(t32).all():
            raise ValueError("threshold must be finite")
        folds = self.kfold(ds, range(0, len(ds)))
        indexes = [int(i) for i in folds.sampledIndexes(fold, False, negatives)]
        if not indexes:
            raise ValueError("fold %r has no validation items" % (fold,))
        m = self.load_model(fold, stage)
        impl = m.impl
        dev, B, C = impl.device, impl.batch, int(self.classes)
        values, reads = (False, True, "d4"), {1: 0, 3: 1, 8: 2}          # the sum after k members is the `values[reads[k]]` prediction
        counts = torch.empty((3, len(indexes), 1, 2), dtype=torch.int64, device=dev)
        totals = torch.empty((3, len(indexes), 2), dtype=torch.int64, device=dev)
        ws = torch.empty(ops.threshold_counts_workspace_bytes(1), dtype=torch.uint8, device=dev)
        for s in range(0, len(indexes), B):
            items = [ds[i] for i in indexes[s:s + B]]
            targets = []
            for it in items:
                y = np.asarray(it.y)
                plane = y if y.ndim == 2 else y[:, :, channel if y.shape[2] > 1 else 0]
                if plane.shape != tuple(it.x.shape[:2]):
                    raise ValueError("item %r: a %s mask for a %d x %d image" % ((it.id, plane.shape) + tuple(it.x.shape[:2])))
                targets.append(torch.from_numpy(np.ascontiguousarray(plane != 0).view(np.uint8)).to(dev))
            xs = self._resize_to_net(impl, [it.x for it in items], device=True)
            for acc, k in self._sum_maps_device([m], "d4", xs, len(items)):
                if k not in reads:
                    continue
                for j, (it, target) in enumerate(zip(items, targets)):
                    h, w = (int(v) for v in it.x.shape[:2])
                    probs = self._new_map(acc, self.PROBS, h, w)
                    ops.predict_finish(acc[j], impl.H, impl.W, C, k, self.PROBS, probs, h, w)
                    ops.threshold_counts(probs, target, h, w, C, channel, t32, counts[reads[k], s + j], totals[reads[k], s + j], ws)
        counts, totals = counts.cpu().numpy(), totals.cpu().numpy()          # the only copies back: 4 integers per image and read
        table = {}
        for v, cn, tt in zip(values, counts, totals):
            if average == "pixels":
                score = self.sweep_score(metric, cn[:, :, 0].sum(0), cn[:, :, 1].sum(0), tt[:, 0].sum())
            else:
                score = self.sweep_score(metric, cn[:, :, 0], cn[:, :, 1], tt[:, :1]).mean(axis=0)
            table[v] = float(score[0])
        return values[int(np.argmax([table[v] for v in values]))], table

    # ---------------------------------------------------------------- object-level scores on the device (csrc/object_match.hip)
    OBJECT_METRICS = ("f2", "ap")
    IOU_DEN = 1000                    # IoU thresholds are exact fractions n / 1000: decimals of up to three places

    @staticmethod
    def object_score(metric, TP, n_pred, n_truth):
        """float64 per-object scores from integer counters (arrays broadcast): TP matched pairs, ``n_pred`` predicted objects, ``n_truth``
        objects of the target; FP = n_pred - TP, FN = n_truth - TP.  ``"f2"`` 5TP / (5TP + 4FN + FP) (Airbus ship detection), ``"ap"``
        TP / (TP + FP + FN) (DSB-2018); 1 where n_pred = n_truth = 0, as ``sweep_score``."""
        if metric not in PipelineConfig.OBJECT_METRICS:
            raise ValueError("metric %r: one of %s" % (metric, ", ".join(PipelineConfig.OBJECT_METRICS)))
        TP, P, G = (np.asarray(a, np.float64) for a in (TP, n_pred, n_truth))
        FP, FN = P - TP, G - TP
        num, den = (5 * TP, 5 * TP + 4 * FN + FP) if metric == "f2" else (TP, TP + FP + FN)
        empty = (P == 0) & (G == 0)
        return np.where(empty, 1.0, num / np.where(empty, 1.0, den))

    @classmethod
    def _iou_fractions(cls, iou_thresholds):
        """-> (numerators, the thresholds as n / 1000): each value a decimal of at most three places in [0.5, 1], strictly ascending, 1 to 64
        of them; default 0.5, 0.55, ..., 0.95."""
        if iou_thresholds is None:
            nums = list(range(500, 1000, 50))
        else:
            nums = []
            for t in iou_thresholds:
                t = float(t)
                n = int(round(t * cls.IOU_DEN)) if np.isfinite(t) else -1
                if n < 0 or abs(t * cls.IOU_DEN - n) > 1e-6:
                    raise ValueError("iou_thresholds are decimals of at most three places: got %r" % (t,))
                nums.append(n)
        if not 1 <= len(nums) <= 64:
            raise ValueError("1 to 64 iou_thresholds: got %d" % len(nums))
        if any(2 * n < cls.IOU_DEN or n > cls.IOU_DEN for n in nums):
            raise ValueError("iou_thresholds lie in [0.5, 1] (below 0.5 an object could have two partners): got %r" % (list(iou_thresholds),))
        if any(b <= a for a, b in zip(nums, nums[1:])):
            raise ValueError("iou_thresholds must be strictly ascending")
        return nums, [n / cls.IOU_DEN for n in nums]

    def _object_args(self, cells, opening, closing, channel, area_threshold, metric, iou_thresholds, truth):
        """The argument checks of the object-score methods, all before a model is loaded -> (mask mode, numerators, thresholds)."""
        if metric not in self.OBJECT_METRICS:
            raise ValueError("metric %r: one of %s" % (metric, ", ".join(self.OBJECT_METRICS)))
        if truth not in ("mask", "labels"):
            raise ValueError("truth %r: 'mask' (objects = the 8-connected components of y != 0) or 'labels' (y[..., 0] numbers them)" % (truth,))
        nums, ts = self._iou_fractions(iou_thresholds)
        mode = 0
        for threshold, min_size in (c[:2] for c in cells):
            mode = self._mask_mode(threshold, opening, closing, channel, min_size, area_threshold)
        return mode, nums, ts

    @staticmethod
    def _truth_labels(it, truth, channel, h, w, dev):
        """The item's ground truth as an int32 device label image [h, w] and the largest value it may hold."""
        import torch
        y = np.asarray(it.y)
        if truth == "labels":
            plane = y if y.ndim == 2 else y[..., 0]
            if plane.shape != (h, w):
                raise ValueError("item %r: a %s label image for a %d x %d image" % (it.id, plane.shape, h, w))
            if plane.dtype.kind not in "iub" or (plane.size and (int(plane.min()) < 0 or int(plane.max()) > h * w)):
                raise ValueError("item %r: truth='labels' takes integer object numbers 0..h * w (0: background)" % (it.id,))
            return torch.from_numpy(np.ascontiguousarray(plane, dtype=np.int32)).to(dev), h * w
        plane = y if y.ndim == 2 else y[:, :, channel if y.shape[2] > 1 else 0]
        if plane.shape != (h, w):
            raise ValueError("item %r: a %s mask for a %d x %d image" % (it.id, plane.shape, h, w))
        mask = torch.from_numpy(np.ascontiguousarray(plane != 0).view(np.uint8)).to(dev)
        return PipelineConfig._device_labels(mask)[0], (h * w + 1) // 2

    def _object_counts(self, ds, fold, stage, negatives, ttflips, cells, mode, opening, closing, channel, area_threshold, nums, truth):
        """-> (ids, int64 [images, cells, T + 3]): per validation item of ``fold`` the network runs once and the truth is labelled once;
        per cell (threshold, min_size) the mask of ``predict_masks_ex``, its 8-connected labels and stp_label_match.  A cell (threshold,
        min_size, c2) scores the split objects instead (``_device_split``; c2 the squared core distance): consecutive cells of one
        (threshold, min_size) share the mask and its stp_mask_edt, so a cell costs the threshold of D2, label, grow and match.  The
        counters stay on the device until the one copy at the end."""
        from segmentation_training_pipeline_amd import ops
        import torch
        self._check_tta(ttflips)
        folds = self.kfold(ds, range(0, len(ds)))
        indexes = [int(i) for i in folds.sampledIndexes(fold, False, negatives)]
        if not indexes:
            raise ValueError("fold %r has no validation items" % (fold,))
        m = self.load_model(fold, stage)
        dev, B, T = m.impl.device, m.impl.batch, len(nums)
        counts = torch.empty((len(indexes), len(cells), T + 3), dtype=torch.int64, device=dev)
        ids = []
        for s in range(0, len(indexes), B):
            items = [ds[i] for i in indexes[s:s + B]]
            for j, (it, probs) in enumerate(zip(items, self._predict_maps_device([m], ttflips, items)[0])):
                h, w = int(probs.shape[0]), int(probs.shape[1])
                ids.append(it.id)
                target, cap = self._truth_labels(it, truth, channel, h, w, dev)
                ws = torch.empty(ops.label_match_workspace_bytes(h, w), dtype=torch.uint8, device=dev)
                shared = (None, None, None)                  # ((threshold, min_size), its mask, its distance transform)
                for c, (threshold, min_size, *c2) in enumerate(cells):
                    if not c2:
                        mask = self._device_mask(probs, mode, float(threshold), int(opening), int(closing), int(channel), int(min_size),
                                                 int(area_threshold))
                        ops.label_match(self._device_labels(mask)[0], target, h, w, cap, nums, self.IOU_DEN, counts[s + j, c], ws)
                        continue
                    if shared[0] != (threshold, min_size):
                        mask = self._device_mask(probs, mode, float(threshold), int(opening), int(closing), int(channel), int(min_size),
                                                 int(area_threshold))
                        shared = ((threshold, min_size), mask, self._device_edt(mask))
                    labels, _ = self._device_split(shared[1], c2[0], shared[2])
                    ops.label_match(labels, target, h, w, h * w, nums, self.IOU_DEN, counts[s + j, c], ws)
        return ids, counts.cpu().numpy()          # the only copy back: T + 3 integers per image and cell

    def score_objects(self, ds, fold, stage=-1, negatives="real", ttflips=None, threshold=0.5, opening=0, closing=0, channel=0, min_size=0,
                      area_threshold=0, metric="f2", iou_thresholds=None, truth="mask"):
        """The per-object competition score of ``predict_masks_ex``'s masks on the validation items of ``fold`` (chosen as ``find_threshold``
        chooses them).  A predicted object - an 8-connected component of the mask, as ``multi_rle_encode`` splits it - is a true positive
        at t when its IoU with an object of the item's mask exceeds t; ``iou_thresholds`` default to 0.5, 0.55, ..., 0.95 (decimals of at
        most three places in [0.5, 1], strictly ascending, compared exactly as n / 1000).  ``metric``: ``"f2"`` (Airbus ship detection)
        or ``"ap"`` (DSB-2018), see ``object_score``.  ``truth="mask"``: the target's objects are the 8-connected components of ``y !=
        0``; ``"labels"``: ``y[..., 0]`` numbers them (integers 0..h * w), so touching objects stay separate.  Per image, all on the
        device: the finished map at the image's own size, the mask (threshold, opening, closing, ``min_size``, ``area_threshold`` - the
        launches of ``predict_masks_ex``), stp_mask_label, the labelled target, stp_label_match; only T + 3 integers per image come
        back, in one copy.  Returns ``{"score": mean over images of the mean over t, "by_iou": {t: mean over images}, "images": [(id,
        score)], "counts": int64 [images, T + 3] = (TP per t, predicted objects, target objects, out-of-range pixels)}``."""
        cells = [(threshold, min_size)]
        mode, nums, ts = self._object_args(cells, opening, closing, channel, area_threshold, metric, iou_thresholds, truth)
        ids, counts = self._object_counts(ds, fold, stage, negatives, ttflips, cells, mode, opening, closing, channel, area_threshold, nums,
                                          truth)
        counts = counts[:, 0]
        T = len(nums)
        per = self.object_score(metric, counts[:, :T], counts[:, T:T + 1], counts[:, T + 1:T + 2])          # [images, T]
        images = per.mean(axis=1)
        return {"score": float(images.mean()), "by_iou": {t: float(v) for t, v in zip(ts, per.mean(axis=0))},
                "images": [(i, float(v)) for i, v in zip(ids, images)], "counts": counts}

    def find_object_threshold(self, ds, fold, stage=-1, negatives="real", ttflips=None, thresholds=None, min_sizes=(0,), opening=0, closing=0,
                              channel=0, area_threshold=0, metric="f2", iou_thresholds=None, truth="mask"):
        """``find_threshold`` for the score the masks are judged on: the cell of the grid ``thresholds`` x ``min_sizes`` - the two
        parameters ``predict_masks_ex`` takes; ``thresholds`` default to d / 20 for d = 1..19 - whose ``score_objects`` is best.  Per
        image the network runs once and the target is labelled once; per cell: threshold (+ opening / closing), area filter, labels,
        stp_label_match.  All counters ([images, cells, T + 3] int64) stay on the device and come back in one copy.  A softmax head
        takes ``channel`` and no ``thresholds``: only ``min_sizes`` are swept.  Returns ``((best_threshold, best_min_size), {(threshold,
        min_size): score})``; the first cell in thresholds-major order wins a tie."""
        if self._softmax_head():
            if thresholds is not None:
                raise ValueError("a softmax head has one label per pixel: the mask of `channel` is argmax == channel and takes no thresholds")
            thresholds = [0.5]
        else:
            thresholds = [d / 20 for d in range(1, 20)] if thresholds is None else [float(t) for t in thresholds]
            t32 = np.asarray(thresholds, np.float32)
            if not 1 <= len(thresholds) <= 64:
                raise ValueError("1 to 64 thresholds in one sweep: got %d" % len(thresholds))
            if not np.isfinite(t32).all() or not (np.diff(t32) > 0).all():
                raise ValueError("thresholds must be finite and strictly ascending (as float32)")
        min_sizes = list(min_sizes)
        if not 1 <= len(min_sizes) <= 64:
            raise ValueError("1 to 64 min_sizes in one sweep: got %d" % len(min_sizes))
        cells = [(t, m) for t in thresholds for m in min_sizes]
        mode, nums, ts = self._object_args(cells, opening, closing, channel, area_threshold, metric, iou_thresholds, truth)
        if any(b <= a for a, b in zip(min_sizes, min_sizes[1:])):
            raise ValueError("min_sizes must be strictly ascending")
        _, counts = self._object_counts(ds, fold, stage, negatives, ttflips, cells, mode, opening, closing, channel, area_threshold, nums,
                                        truth)
        T = len(nums)
        per = self.object_score(metric, counts[:, :, :T], counts[:, :, T:T + 1], counts[:, :, T + 1:T + 2])   # [images, cells, T]
        scores = [float(np.ascontiguousarray(per[:, c]).mean(axis=1).mean()) for c in range(len(cells))]      # score_objects' own sums
        table = dict(zip(cells, scores))
        return cells[int(np.argmax(scores))], table

    @staticmethod
    def object_overlaps(pred_labels, truth_labels):
        """The overlap table of two integer label images [h, w] (numpy, 0 = background, values 0..h * w) for custom object metrics ->
        ``(pairs, area_pred, area_truth)``: ``pairs`` int32 [k, 3] = (a, b, pixels with pred = a and truth = b) for every pair that shares
        a pixel, sorted by (a, b); ``area_*`` int32 [max label + 1] = the labels' pixel counts.  stp_label_overlaps on the device."""
        from segmentation_training_pipeline_amd import ops
        import torch
        p, g = np.asarray(pred_labels), np.asarray(truth_labels)
        if p.ndim != 2 or p.shape != g.shape or p.size == 0 or p.dtype.kind not in "iub" or g.dtype.kind not in "iub":
            raise ValueError("object_overlaps takes two non-empty integer label images of one shape [h, w]")
        h, w = p.shape
        cap = int(max(p.max(), g.max()))
        if int(min(p.min(), g.min())) < 0 or cap > h * w:
            raise ValueError("labels are object numbers 0..h * w (0: background)")
        dev = "cuda"
        pd, gd = (torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev) for a in (p, g))
        triples = torch.empty((h * w, 3), dtype=torch.int32, device=dev)
        count = torch.empty(1, dtype=torch.int32, device=dev)
        areas = torch.empty((2, cap + 1), dtype=torch.int32, device=dev)
        outside = torch.empty(1, dtype=torch.int64, device=dev)
        ws = torch.empty(ops.label_overlaps_workspace_bytes(h, w), dtype=torch.uint8, device=dev)
        ops.label_overlaps(pd, gd, h, w, cap, triples, count, areas[0], areas[1], outside, ws)
        pairs = triples[:int(count.item())].cpu().numpy()
        pairs = pairs[np.lexsort((pairs[:, 1], pairs[:, 0]))]          # the device's order is unspecified: sorted by (a, b)
        areas = areas.cpu().numpy()
        return pairs, areas[0], areas[1]

    # ---------------------------------------------------------------- touching objects split on the device (csrc/split.hip)
    MAX_SPLIT = 1024

    @classmethod
    def _split_c2(cls, split):
        """The squared core distance floor(r * r) of the public radius ``split``: a real, finite number in 0..1024, not a bool."""
        if isinstance(split, (bool, np.bool_)) or not isinstance(split, (int, float, np.integer, np.floating)):
            raise ValueError("split is the radius of the cores, a number in 0..%d (0: off): got %r" % (cls.MAX_SPLIT, split))
        r = float(split)
        if not np.isfinite(r) or not 0 <= r <= cls.MAX_SPLIT:
            raise ValueError("split is the radius of the cores, a finite number in 0..%d (0: off): got %r" % (cls.MAX_SPLIT, split))
        return int(np.floor(r * r))

    @staticmethod
    def _device_edt(mask):
        """-> int32 device image [h, w]: stp_mask_edt of a device mask, the exact squared distance to the nearest zero pixel."""
        from segmentation_training_pipeline_amd import ops
        import torch
        h, w = (int(v) for v in mask.shape)
        d2 = torch.empty((h, w), dtype=torch.int32, device=mask.device)
        ws = torch.empty(ops.mask_edt_workspace_bytes(h, w), dtype=torch.uint8, device=mask.device)
        ops.mask_edt(mask, h, w, d2, ws)
        return d2

    @classmethod
    def _device_split(cls, mask, c2, d2=None):
        """-> (int32 device label image [h, w], device count [1]): the objects of a device mask with every component cut at its necks.
        The cores ``d2 > c2`` (``d2``: the mask's ``_device_edt``, computed here when None) are numbered by stp_mask_label (connectivity
        2) and grown back through the mask by stp_label_grow - a pixel takes the core that reaches it first over the 8-neighbourhood,
        the smaller number on a tie -; the components no core reached are numbered after them (stp_label_unclaimed, stp_mask_label,
        stp_label_merge).  The only values read on the host are stp_label_grow's "changed" words, one per call."""
        from segmentation_training_pipeline_amd import ops
        import torch
        h, w = (int(v) for v in mask.shape)
        if d2 is None:
            d2 = cls._device_edt(mask)
        part = torch.empty((h, w), dtype=torch.uint8, device=mask.device)
        ops.edt_threshold(d2, h, w, c2, part)
        labels, nc = cls._device_labels(part)
        words = torch.empty(2, dtype=torch.int32, device=mask.device)
        ws = torch.empty(ops.label_grow_workspace_bytes(h, w), dtype=torch.uint8, device=mask.device)
        ops.label_grow(mask, labels, h, w, labels, words[:1], ws)
        ops.label_unclaimed(mask, labels, h, w, part)
        rest, nr = cls._device_labels(part)
        ops.label_merge(rest, nc, nr, h, w, labels, words[1:])
        return labels, words[1:]

    @staticmethod
    def split_labels(mask, split):
        """The split objects of a numpy mask [h, w] (any non-zero value is foreground) for custom code -> ``(int32 label image, count)``:
        what ``predict_instances(rle=False, split=split)`` makes of its mask, on the device.  ``split=0``: scipy.ndimage.label with the
        8-neighbourhood."""
        import torch
        c2 = PipelineConfig._split_c2(split)
        m = np.asarray(mask)
        if m.ndim != 2 or m.size == 0 or m.dtype.kind not in "iubf":
            raise ValueError("split_labels takes a non-empty numeric mask [h, w]")
        dm = torch.from_numpy(np.ascontiguousarray(m != 0).view(np.uint8)).to("cuda")
        labels, count = PipelineConfig._device_split(dm, c2)
        return labels.cpu().numpy(), int(count.item())

    @staticmethod
    def border_weight_map(mask, w0=10, sigma=5, radius=None, class_balance=(1, 1), labelled=False):
        """The U-Net border weight map of a numpy mask [h, w] -> float32 [h, w], computed on the device by the launches a model with the
        ``border_weights`` key runs per step (stp_mask_label with the 8-neighbourhood, stp_border_weight): ``class_balance[1]`` on the
        objects, ``class_balance[0]`` on the background plus ``w0 * exp(-(d1 + d2)^2 / (2 sigma^2))`` where two objects lie within
        ``radius`` (default ceil(4 sigma), at most 32) of the pixel.  ``labelled=True``: ``mask`` is an instance label image (integers, 0 =
        background) and is taken as it is - touching instances with different labels get a border between them."""
        import torch
        from segmentation_training_pipeline_amd import backend, ops
        p = backend.border_weight_params(w0, sigma, radius, class_balance)
        m = np.asarray(mask)
        if m.ndim != 2 or m.size == 0 or m.dtype.kind not in "iubf":
            raise ValueError("border_weight_map takes a non-empty numeric mask [h, w]")
        h, w = (int(v) for v in m.shape)
        if labelled:
            if m.dtype.kind not in "iub" or (m.dtype.kind == "i" and int(m.min()) < 0) or int(m.max()) > 2 ** 31 - 1:
                raise ValueError("border_weight_map(labelled=True) takes an integer label image with values 0..2^31 - 1")
            labels = torch.from_numpy(np.ascontiguousarray(m).astype(np.int32)).to("cuda")
        else:
            labels, _ = PipelineConfig._device_labels(torch.from_numpy(np.ascontiguousarray(m != 0).view(np.uint8)).to("cuda"))
        out = torch.empty((h, w), dtype=torch.float32, device=labels.device)
        ws = torch.empty(ops.border_weight_workspace_bytes(1, h, w), dtype=torch.uint8, device=labels.device)
        ops.border_weight(labels, 1, h, w, p["w0"], p["sigma"], p["radius"], p["class_balance"][0], p["class_balance"][1], out, ws)
        return out.cpu().numpy()

    def predict_instances(self, spath, fold=0, stage=0, limit=-1, ttflips=False, threshold=0.5, opening=0, closing=0, channel=0, rle=True,
                          min_size=0, area_threshold=0, split=0.0):
        """``predict_masks_ex(components=True)`` with touching objects kept apart: a generator of ``(file_name, [rle_string, ...])``, one
        string per object in label order - or, ``rle=False``, ``(file_name, int32 h x w label image)``.  Per image the launches of
        ``predict_masks_ex`` make the mask; then every 8-connected component is cut at its necks: the pixels farther than ``split``
        from the background (exact Euclidean distance; ``split`` a radius in pixels, 0..1024) form the cores, which are numbered in
        scipy's order and grown back through the mask - a pixel joins the core that reaches it first over the 8-neighbourhood, the
        smaller number on a tie -, and a component without a core stays one object, numbered after the cores.  ``split=0`` is
        ``components=True`` bit for bit.  Unlike a larger ``opening`` this removes no pixel: the objects partition the mask."""
        mode = self._mask_mode(threshold, opening, closing, channel, min_size, area_threshold)      # (refusals fire here, not at the first next())
        self._check_tta(ttflips)
        c2 = self._split_c2(split)

        def instances():
            for items, maps in self._predict_batches(spath, fold, stage, limit, ttflips, self.PROBS, device=True):
                for it, probs in zip(items, maps):
                    mask = self._device_mask(probs, mode, float(threshold), int(opening), int(closing), int(channel), int(min_size),
                                             int(area_threshold))
                    labels, count = self._device_split(mask, c2)
                    yield it.id, (self._device_label_codes(labels, count) if rle else labels.cpu().numpy())
        return instances()

    def predict_instances_to_csv(self, spath, csv_path, fold=0, stage=0, limit=-1, ttflips=False, threshold=0.5, opening=0, closing=0,
                                 channel=0, columns=("image", "rle_mask"), min_size=0, area_threshold=0, split=0.0):
        """``predict_instances`` written as ``predict_to_csv(components=True)`` writes its objects: one row per object, the image name
        repeated; an image without objects gets one row with an empty code.  Returns the number of rows."""
        if len(columns) != 2:
            raise ValueError("columns names the image column and the run-length column")
        rows = self.predict_instances(spath, fold, stage, limit, ttflips, threshold, opening, closing, channel, True, min_size, area_threshold,
                                      split)
        return self._write_csv(csv_path, columns, rows, True)

    def score_instances(self, ds, fold, stage=-1, negatives="real", ttflips=None, threshold=0.5, opening=0, closing=0, channel=0, min_size=0,
                        area_threshold=0, metric="f2", iou_thresholds=None, truth="mask", split=0.0):
        """``score_objects`` of ``predict_instances``' objects: the same arguments, then ``split``; the same dict.  The target is handled
        exactly as there (``truth="mask"`` / ``"labels"``) and is never split.  ``split=0`` gives ``score_objects``' counters."""
        cells = [(threshold, min_size, self._split_c2(split))]
        mode, nums, ts = self._object_args(cells, opening, closing, channel, area_threshold, metric, iou_thresholds, truth)
        ids, counts = self._object_counts(ds, fold, stage, negatives, ttflips, cells, mode, opening, closing, channel, area_threshold, nums,
                                          truth)
        counts = counts[:, 0]
        T = len(nums)
        per = self.object_score(metric, counts[:, :T], counts[:, T:T + 1], counts[:, T + 1:T + 2])          # [images, T]
        images = per.mean(axis=1)
        return {"score": float(images.mean()), "by_iou": {t: float(v) for t, v in zip(ts, per.mean(axis=0))},
                "images": [(i, float(v)) for i, v in zip(ids, images)], "counts": counts}

    def find_split(self, ds, fold, stage=-1, negatives="real", ttflips=None, thresholds=None, splits=(0, 2, 4, 6), min_size=0, opening=0,
                   closing=0, channel=0, area_threshold=0, metric="f2", iou_thresholds=None, truth="mask"):
        """``find_object_threshold`` over the grid ``thresholds`` x ``splits`` (1 to 64 radii, strictly ascending): the cell whose
        ``score_instances`` is best.  Per image the network runs once and the target is labelled once; per threshold the mask and its
        distance transform are made once; per split only the threshold of the distances, the labels, the growth and stp_label_match
        run.  A softmax head takes ``channel`` and no ``thresholds``.  Returns ``((best_threshold, best_split), {(threshold, split):
        score})``; the first cell in thresholds-major order wins a tie."""
        if self._softmax_head():
            if thresholds is not None:
                raise ValueError("a softmax head has one label per pixel: the mask of `channel` is argmax == channel and takes no thresholds")
            thresholds = [0.5]
        else:
            thresholds = [d / 20 for d in range(1, 20)] if thresholds is None else [float(t) for t in thresholds]
            t32 = np.asarray(thresholds, np.float32)
            if not 1 <= len(thresholds) <= 64:
                raise ValueError("1 to 64 thresholds in one sweep: got %d" % len(thresholds))
            if not np.isfinite(t32).all() or not (np.diff(t32) > 0).all():
                raise ValueError("thresholds must be finite and strictly ascending (as float32)")
        splits = list(splits)
        if not 1 <= len(splits) <= 64:
            raise ValueError("1 to 64 splits in one sweep: got %d" % len(splits))
        c2s = [self._split_c2(r) for r in splits]
        if any(b <= a for a, b in zip(splits, splits[1:])):
            raise ValueError("splits must be strictly ascending")
        keys = [(t, r) for t in thresholds for r in splits]
        cells = [(t, min_size, c2) for t in thresholds for c2 in c2s]
        mode, nums, ts = self._object_args(cells, opening, closing, channel, area_threshold, metric, iou_thresholds, truth)
        _, counts = self._object_counts(ds, fold, stage, negatives, ttflips, cells, mode, opening, closing, channel, area_threshold, nums,
                                        truth)
        T = len(nums)
        per = self.object_score(metric, counts[:, :, :T], counts[:, :, T:T + 1], counts[:, :, T + 1:T + 2])   # [images, cells, T]
        scores = [float(np.ascontiguousarray(per[:, c]).mean(axis=1).mean()) for c in range(len(cells))]      # score_instances' own sums
        table = dict(zip(keys, scores))
        return keys[int(np.argmax(scores))], table

    # ---------------------------------------------------------------- per-object measurements on the device (csrc/measure.hip)
    CONF_ONE = 65535                  # the fixed-point probability of a pixel: q = (int)(clamp(p, 0, 1) * 65535)
    CONF_DEN = 10000                  # min_confidence is an exact fraction n / 10000: a decimal of up to four places
    MEASURES = ("area", "confidence", "y0", "x0", "y1", "x1", "cy", "cx")

    @classmethod
    def _conf_num(cls, min_confidence, name="min_confidence"):
        """The numerator n of ``min_confidence`` = n / 10000: a real number in [0, 1] with at most four decimal places, not a bool."""
        t = min_confidence
        if isinstance(t, (bool, np.bool_)) or not isinstance(t, (int, float, np.integer, np.floating)):
            raise ValueError("%s is a decimal of at most four places in [0, 1]: got %r" % (name, t))
        t = float(t)
        n = int(round(t * cls.CONF_DEN)) if np.isfinite(t) else -1
        if n < 0 or n > cls.CONF_DEN or abs(t * cls.CONF_DEN - n) > 1e-6:
            raise ValueError("%s is a decimal of at most four places in [0, 1]: got %r" % (name, min_confidence))
        return n

    @staticmethod
    def _min_area(min_area):
        if isinstance(min_area, (bool, np.bool_)) or not isinstance(min_area, (int, np.integer)) or min_area < 0:
            raise ValueError("min_area is a pixel count, an integer >= 0 (0: off): got %r" % (min_area,))
        return int(min_area)

    @staticmethod
    def object_table(sums, boxes, count):
        """The per-object table of stp_label_measure's integers (``sums`` int64 [rows, 4] = area, sum y, sum x, sum q; ``boxes`` int32 [rows,
        4] = the closed box) over the objects 1..count -> a dict of numpy arrays: ``label``, ``area`` and the half-open box ``y0``, ``x0``,
        ``y1``, ``x1`` (scipy.ndimage.find_objects' slices) as int64; the centroid ``cy``, ``cx`` and ``confidence`` = sum q / (65535 *
        area), the object's mean probability, as float64 (NaN for a label without a pixel)."""
        s, b = np.asarray(sums, np.int64)[1:count + 1], np.asarray(boxes, np.int64)[1:count + 1]
        area = s[:, 0].astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            return {"label": np.arange(1, count + 1, dtype=np.int64), "area": s[:, 0].copy(), "y0": b[:, 0].copy(), "x0": b[:, 1].copy(),
                    "y1": b[:, 2] + 1, "x1": b[:, 3] + 1, "cy": s[:, 1] / area, "cx": s[:, 2] / area,
                    "confidence": s[:, 3] / (np.float64(PipelineConfig.CONF_ONE) * area)}

    @staticmethod
    def _device_measure(labels, cap, probs=None, channel=0):
        """-> (int64 sums [cap + 1, 4], int32 boxes [cap + 1, 4], int64 out-of-range count [1]), all on the device: stp_label_measure of
        a device label image with values 0..cap and, optionally, the float32 device map [h, w, C]."""
        from segmentation_training_pipeline_amd import ops
        import torch
        h, w = (int(v) for v in labels.shape)
        sums = torch.empty((cap + 1, 4), dtype=torch.int64, device=labels.device)
        boxes = torch.empty((cap + 1, 4), dtype=torch.int32, device=labels.device)
        outside = torch.empty(1, dtype=torch.int64, device=labels.device)
        ops.label_measure(labels, probs, h, w, 1 if probs is None else int(probs.shape[2]), int(channel), cap, sums, boxes, outside)
        return sums, boxes, outside

    @classmethod
    def _device_select(cls, labels, cap, sums, boxes, min_area, num, out=None):
        """-> (int32 device label image, device count [1], sums, boxes): stp_label_select - the objects with ``area >= min_area`` and mean
        probability >= num / 10000, renumbered in order, and their rows.  ``out``: the buffers of an earlier call of the same shape."""
        from segmentation_training_pipeline_amd import ops
        import torch
        h, w = (int(v) for v in labels.shape)
        if out is None:
            out = (torch.empty_like(labels), torch.empty(1, dtype=torch.int32, device=labels.device), torch.empty_like(sums),
                   torch.empty_like(boxes), torch.empty(ops.label_select_workspace_bytes(cap), dtype=torch.uint8, device=labels.device))
        ops.label_select(labels, h, w, cap, sums, boxes, min_area, num, cls.CONF_DEN, out[0], out[1], out[2], out[3], out[4])
        return out

    @staticmethod
    def measure_labels(labels, probs=None, channel=0):
        """The per-object table of a numpy label image [h, w] (integers 0..h * w, 0 = background) for custom code, on the device: the
        ``object_table`` dict over the labels 1..labels.max() - a value that does not occur has area 0 - plus ``"out_of_range"``.
        ``probs``: a numpy map [h, w] or [h, w, C] whose ``channel`` gives the confidence; None: confidence 0."""
        import torch
        lab = np.asarray(labels)
        if lab.ndim != 2 or lab.size == 0 or lab.dtype.kind not in "iub":
            raise ValueError("measure_labels takes a non-empty integer label image [h, w]")
        h, w = lab.shape
        cap = int(lab.max())
        if int(lab.min()) < 0 or cap > h * w:
            raise ValueError("labels are object numbers 0..h * w (0: background)")
        dp = None
        if probs is not None:
            p = np.asarray(probs)
            if p.dtype.kind not in "fiub" or p.ndim not in (2, 3) or p.shape[:2] != (h, w) or (p.ndim == 3 and p.shape[2] < 1):
                raise ValueError("probs is a numeric map [h, w] or [h, w, C] of the label image's size")
            p = p[:, :, None] if p.ndim == 2 else p
            if isinstance(channel, (bool, np.bool_)) or not isinstance(channel, (int, np.integer)) or not 0 <= channel < p.shape[2]:
                raise ValueError("channel %r: the map has %d channel(s)" % (channel, p.shape[2]))
            dp = torch.from_numpy(np.ascontiguousarray(p, dtype=np.float32)).to("cuda")
        dl = torch.from_numpy(np.ascontiguousarray(lab, dtype=np.int32)).to("cuda")
        sums, boxes, outside = PipelineConfig._device_measure(dl, cap, dp, int(channel) if dp is not None else 0)
        out = PipelineConfig.object_table(sums.cpu().numpy(), boxes.cpu().numpy(), cap)
        out["out_of_range"] = int(outside.item())
        return out

    def predict_instances_ex(self, spath, fold=0, stage=0, limit=-1, ttflips=False, threshold=0.5, opening=0, closing=0, channel=0, rle=True,
                             min_size=0, area_threshold=0, split=0.0, min_area=0, min_confidence=0.0, measure=False):
        """``predict_instances`` (same arguments, and exactly its launches and results when the three new keywords keep their defaults)
        with the objects then measured and selected on the device: after the split, stp_label_measure takes every object's area, bounding
        box, centroid sums and the sum of ``probs[..., channel]`` of the finished map at the image's own size in 1 / 65535 units;
        stp_label_select keeps the objects with at least ``min_area`` pixels (an integer >= 0; unlike ``min_size`` it also sees the
        fragments a split creates) whose mean probability is at least ``min_confidence`` (a decimal of at most four places in [0, 1],
        compared exactly as n / 10000) and renumbers them in order.  Yields ``(file_name, codes_or_labels)`` or, ``measure=True``,
        ``(file_name, codes_or_labels, table)`` with ``table`` the ``object_table`` dict of the objects that are left."""
        mode = self._mask_mode(threshold, opening, closing, channel, min_size, area_threshold)      # (refusals fire here, not at the first next())
        self._check_tta(ttflips)
        c2 = self._split_c2(split)
        min_area, num = self._min_area(min_area), self._conf_num(min_confidence)
        if not (min_area or num or measure):
            return self.predict_instances(spath, fold, stage, limit, ttflips, threshold, opening, closing, channel, rle, min_size,
                                          area_threshold, split)

        def instances():
            for items, maps in self._predict_batches(spath, fold, stage, limit, ttflips, self.PROBS, device=True):
                for it, probs in zip(items, maps):
                    mask = self._device_mask(probs, mode, float(threshold), int(opening), int(closing), int(channel), int(min_size),
                                             int(area_threshold))
                    labels, count = self._device_split(mask, c2)
                    n = int(count.item())
                    sums, boxes, _ = self._device_measure(labels, n, probs, int(channel))
                    if min_area or num:                       # (the split's labels are 1..n, each with a pixel: nothing else to drop)
                        labels, count, sums, boxes, _ = self._device_select(labels, n, sums, boxes, min_area, num)
                        n = int(count.item())
                    out = self._device_label_codes(labels, count) if rle else labels.cpu().numpy()
                    if measure:
                        yield it.id, out, self.object_table(sums[:n + 1].cpu().numpy(), boxes[:n + 1].cpu().numpy(), n)
                    else:
                        yield it.id, out
        return instances()

    @classmethod
    def _measure_names(cls, columns, measures):
        if len(columns) != 2:
            raise ValueError("columns names the image column and the run-length column")
        if isinstance(measures, str) or any(m not in cls.MEASURES for m in measures):
            raise ValueError("measures is a tuple of names from %s: got %r" % (", ".join(cls.MEASURES), measures))
        return tuple(measures)

    def predict_instances_to_csv_ex(self, spath, csv_path, fold=0, stage=0, limit=-1, ttflips=False, threshold=0.5, opening=0, closing=0,
                                    channel=0, columns=("image", "rle_mask"), min_size=0, area_threshold=0, split=0.0, min_area=0,
                                    min_confidence=0.0, measures=()):
        """``predict_instances_ex`` written as ``predict_instances_to_csv`` writes its objects, with the columns named in ``measures`` (a tuple
        of names from ``"area", "confidence", "y0", "x0", "y1", "x1", "cy", "cx"``, which are also their headers) appended: integers as
        integers, floats with ``repr``.  An image without objects gets one row whose other fields are empty.  Returns the number of rows."""
        import csv
        measures = self._measure_names(columns, measures)
        rows = self.predict_instances_ex(spath, fold, stage, limit, ttflips, threshold, opening, closing, channel, True, min_size,
                                         area_threshold, split, min_area, min_confidence, True)
        n = 0
        with open(csv_path, "w", newline="") as f:
            out = csv.writer(f, lineterminator="\n")
            out.writerow(list(columns) + list(measures))
            for name, codes, table in rows:
                stem = name[0:name.index(".")] if "." in name else name
                for k, code in enumerate(codes):
                    cells = [table[m][k] for m in measures]
                    out.writerow([stem, code] + [repr(float(v)) if isinstance(v, np.floating) else str(int(v)) for v in cells])
                    n += 1
                if not codes:
                    out.writerow([stem] + [""] * (1 + len(measures)))
                    n += 1
        return n

    def _selected_counts(self, ds, fold, stage, negatives, ttflips, cells, mode, opening, closing, channel, area_threshold, nums, truth):
        """``_object_counts`` for cells (threshold, min_size, c2, min_area, conf_num) -> (ids, int64 [images, cells, T + 3]).  Per validation
        item of ``fold`` the network runs once and the truth is labelled once; consecutive cells of one (threshold, min_size, c2) share the
        mask, its split and ONE stp_label_measure; a cell costs stp_label_select and stp_label_match (a cell that selects nothing away
        matches the shared labels as they are).  The counters stay on the device until the one copy at the end."""
        from segmentation_training_pipeline_amd import ops
        import torch
        self._check_tta(ttflips)
        folds = self.kfold(ds, range(0, len(ds)))
        indexes = [int(i) for i in folds.sampledIndexes(fold, False, negatives)]
        if not indexes:
            raise ValueError("fold %r has no validation items" % (fold,))
        m = self.load_model(fold, stage)
        dev, B, T = m.impl.device, m.impl.batch, len(nums)
        counts = torch.empty((len(indexes), len(cells), T + 3), dtype=torch.int64, device=dev)
        ids = []
        for s in range(0, len(indexes), B):
            items = [ds[i] for i in indexes[s:s + B]]
            for j, (it, probs) in enumerate(zip(items, self._predict_maps_device([m], ttflips, items)[0])):
                h, w = int(probs.shape[0]), int(probs.shape[1])
                ids.append(it.id)
                target, _ = self._truth_labels(it, truth, channel, h, w, dev)
                ws = torch.empty(ops.label_match_workspace_bytes(h, w), dtype=torch.uint8, device=dev)
                cap = h * w                                  # (the object count stays on the device: the most an image can hold)
                shared, table, out = None, None, None        # (threshold, min_size, c2), (its labels, sums, boxes), the selection's buffers
                for c, (threshold, min_size, c2, min_area, num) in enumerate(cells):
                    if shared != (threshold, min_size, c2):
                        mask = self._device_mask(probs, mode, float(threshold), int(opening), int(closing), int(channel), int(min_size),
                                                 int(area_threshold))
                        labels = self._device_split(mask, c2)[0] if c2 else self._device_labels(mask)[0]
                        shared, table = (threshold, min_size, c2), None
                    chosen = labels
                    if min_area or num:
                        if table is None:
                            table = self._device_measure(labels, cap, probs, int(channel))
                        out = self._device_select(labels, cap, table[0], table[1], min_area, num, out)
                        chosen = out[0]
                    ops.label_match(chosen, target, h, w, cap, nums, self.IOU_DEN, counts[s + j, c], ws)
        return ids, counts.cpu().numpy()          # the only copy back: T + 3 integers per image and cell

    def score_instances_ex(self, ds, fold, stage=-1, negatives="real", ttflips=None, threshold=0.5, opening=0, closing=0, channel=0,
                           min_size=0, area_threshold=0, metric="f2", iou_thresholds=None, truth="mask", split=0.0, min_area=0,
                           min_confidence=0.0):
        """``score_instances`` of ``predict_instances_ex``' objects: the same arguments, then ``min_area`` and ``min_confidence``; the same
        dict.  With both at 0 the counters are ``score_instances``' own."""
        cells = [(threshold, min_size, self._split_c2(split), self._min_area(min_area), self._conf_num(min_confidence))]
        mode, nums, ts = self._object_args(cells, opening, closing, channel, area_threshold, metric, iou_thresholds, truth)
        ids, counts = self._selected_counts(ds, fold, stage, negatives, ttflips, cells, mode, opening, closing, channel, area_threshold, nums,
                                            truth)
        counts = counts[:, 0]
        T = len(nums)
        per = self.object_score(metric, counts[:, :T], counts[:, T:T + 1], counts[:, T + 1:T + 2])          # [images, T]
        images = per.mean(axis=1)
        return {"score": float(images.mean()), "by_iou": {t: float(v) for t, v in zip(ts, per.mean(axis=0))},
                "images": [(i, float(v)) for i, v in zip(ids, images)], "counts": counts}

    def find_confidence(self, ds, fold, stage=-1, negatives="real", ttflips=None, thresholds=None, confidences=(0.0, 0.5, 0.6, 0.7, 0.8),
                        split=0.0, min_size=0, min_area=0, opening=0, closing=0, channel=0, area_threshold=0, metric="f2",
                        iou_thresholds=None, truth="mask"):
        """``find_split`` over the grid ``thresholds`` x ``confidences`` (1 to 64 decimals of at most four places in [0, 1], strictly
        ascending): the cell whose ``score_instances_ex`` is best.  Per image the network runs once and the target is labelled once; per
        threshold the mask, its split and one stp_label_measure run once; per confidence only stp_label_select and stp_label_match run.
        A softmax head takes ``channel`` and no ``thresholds``.  Returns ``((best_threshold, best_confidence), {(threshold, confidence):
        score})``; the first cell in thresholds-major order wins a tie."""
        if self._softmax_head():
            if thresholds is not None:
                raise ValueError("a softmax head has one label per pixel: the mask of `channel` is argmax == channel and takes no thresholds")
            thresholds = [0.5]
        else:
            thresholds = [d / 20 for d in range(1, 20)] if thresholds is None else [float(t) for t in thresholds]
            t32 = np.asarray(thresholds, np.float32)
            if not 1 <= len(thresholds) <= 64:
                raise ValueError("1 to 64 thresholds in one sweep: got %d" % len(thresholds))
            if not np.isfinite(t32).all() or not (np.diff(t32) > 0).all():
                raise ValueError("thresholds must be finite and strictly ascending (as float32)")
        confidences = list(confidences)
        if not 1 <= len(confidences) <= 64:
            raise ValueError("1 to 64 confidences in one sweep: got %d" % len(confidences))
        conf_nums = [self._conf_num(v, "confidences") for v in confidences]
        if any(b <= a for a, b in zip(conf_nums, conf_nums[1:])):
            raise ValueError("confidences must be strictly ascending")
        c2, min_area = self._split_c2(split), self._min_area(min_area)
        keys = [(t, v) for t in thresholds for v in confidences]
        cells = [(t, min_size, c2, min_area, n) for t in thresholds for n in conf_nums]
        mode, nums, ts = self._object_args(cells, opening, closing, channel, area_threshold, metric, iou_thresholds, truth)
        _, counts = self._selected_counts(ds, fold, stage, negatives, ttflips, cells, mode, opening, closing, channel, area_threshold, nums,
                                          truth)
        T = len(nums)
        per = self.object_score(metric, counts[:, :, :T], counts[:, :, T:T + 1], counts[:, :, T + 1:T + 2])   # [images, cells, T]
        scores = [float(np.ascontiguousarray(per[:, c]).mean(axis=1).mean()) for c in range(len(cells))]      # score_instances_ex' own sums
        table = dict(zip(keys, scores))
        return keys[int(np.argmax(scores))], table


class PredictedMap(object):
    """What callbacks receive in place of imgaug's SegmentationMapOnImage: ``.arr`` is the HxWxC array."""

    def __init__(self, arr):
        self.arr = arr
        self.shape = arr.shape


class EvalBatch(object):
    """Stand-in for imgaug.Batch as produced by evaluateAll (reference :184-186)."""

    def __init__(self, images, data, segmentation_maps, predicted_maps_aug):
        self.images, self.data = images, data
        self.segmentation_maps, self.predicted_maps_aug = segmentation_maps, predicted_maps_aug


def parse(path) -> PipelineConfig:
    cfg = PipelineConfig(**generic.load_yaml(path))
    cfg.path = path
    return cfg
