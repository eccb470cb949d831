"""On-the-fly augmentation on the device: the reference's `deepsvg.svg_dataset` - the loader its README names for a user's own
icons - at the seam `deepsvg/train.py:25-28` uses:

    cfg.dataloader_module  = "deepsvg_amd.svg_dataset"
    cfg.collate_fn         = deepsvg_amd.dataset.device_collate
    cfg.loader_num_workers = 0
    cfg.data_dir           = a directory that holds svg_store.npz (or the file itself)

The reference parses an `.svg` file per item and runs ``SVGDataset.preprocess`` on Python objects: a random zoom about the
view-box centre, a random translation, ``SVG.numericalize(256)`` (svg_dataset.py:137-172), then the cat / pad chain of
`get_data`.  Here the icons live in HBM as one float32 PackedSVGStore (deepsvg_amd/dataset.py: raw coordinates in the store's
view box, e.g. `PackedSVGStore.from_batch` over what `paths.canonicalize` / `paths.simplify_heuristic` return), the draws are
made by the torch generator on the device, and ONE kernel launch per layout (dsvg_assemble_augmented) transforms, rounds
and frames every row of the batch: fresh augmentation for every batch, no host round trip, no Python object per icon.  The
arithmetic is the reference's, float32 operation by float32 operation (`paths.transform`); tests/golden/paths/transform.npz
compares the batches with the reference's own by equality.

Kept from the reference's surface: `SVGDataset(..., model_args, max_num_groups, max_seq_len, max_total_len, PAD_VAL,
nb_augmentations)`, `get`, `__getitem__`, `__len__ = n_icons * nb_augmentations`, `random_icon`, `preprocess`-equivalent
switches (`random_aug=False` is ``preprocess(augment=False)``: the numericalize chain only), the `get_data` keys ("commands",
"args", "args_rel", their "_grouped" forms, "filling", "label"), `load_dataset(cfg)`.  Not carried over: reading `.svg` text
(`_load_svg`, the `svg=` argument of `get`) stays with the reference's svglib - parse there once, hand the tensors to
`PackedSVGStore.from_icons(numericalized=False)` or to the `paths` chain - and the "tensor" keys.
"""
import os

import torch
import torch.utils.data

from . import ops, paths
from .dataset import PackedSVGStore, _Deferred, device_collate      # noqa: F401  (device_collate: the collate_fn of the seam)
from .lib import DsvgError

STORE_FILE = "svg_store.npz"


class SVGDataset(torch.utils.data.Dataset):
    """A float32 PackedSVGStore with the reference's augmentation applied as batches are assembled.  `store=` is the store
    (host or device); `device=` where it is to live; `deferred=True` makes `__getitem__` hand the index to
    `dataset.device_collate` (one launch per batch)."""

    def __init__(self, store=None, model_args=None, max_num_groups=8, max_seq_len=30, max_total_len=None, PAD_VAL=-1,
                 device="cuda", deferred=False, nb_augmentations=1, args_dim=256):
        if store is None or not store.is_float:
            raise DsvgError("SVGDataset reads a float32 PackedSVGStore (from_icons(numericalized=False) or from_batch); "
                            "numericalised int16 stores belong to deepsvg_amd.dataset.SVGTensorDataset")
        self.MAX_NUM_GROUPS = max_num_groups
        self.MAX_SEQ_LEN = max_seq_len
        self.MAX_TOTAL_LEN = max_total_len if max_total_len is not None else max_num_groups * max_seq_len
        self.model_args = model_args
        self.PAD_VAL = PAD_VAL
        self.ARGS_DIM = int(args_dim)
        self.deferred = deferred
        self.nb_augmentations = int(nb_augmentations)
        if store.G != max_num_groups:
            raise DsvgError(f"store was packed for {store.G} groups, dataset asks for {max_num_groups}")
        if store.max_group_len > self.MAX_SEQ_LEN or store.max_total_len > self.MAX_TOTAL_LEN:
            raise DsvgError(f"store holds groups of {store.max_group_len} / icons of {store.max_total_len} commands; "
                            f"limits are max_seq_len={self.MAX_SEQ_LEN}, max_total_len={self.MAX_TOTAL_LEN}")
        self.store = store if store.is_device else store.to(device)
        self.device = self.store.rows.device
        self._gen = None
        # the two chains of `preprocess`, packed once: the step kinds and the constant parameters [1, K, 3]; a batch fills in
        # its draws (step 1: the zoom factor, step 3: the translation) with two device copies
        vb, n = self.store.viewbox, self.ARGS_DIM
        plain = paths._normalize_steps("SVGDataset", vb, n)
        augmented = paths._zoom_steps("SVGDataset", 1.0, None, vb) + [("translate", (0.0, 0.0))] + plain
        self._chains = {False: paths._pack_steps("SVGDataset", plain, 1, self.device),
                        True: paths._pack_steps("SVGDataset", augmented, 1, self.device)}

    def __len__(self):
        return self.store.n_icons * self.nb_augmentations

    def idx_to_id(self, idx):
        return self.store.ids[idx] if self.store.ids is not None else idx

    def manual_seed(self, seed):
        """seed of the augmentation draws (the reference draws them from python's `random`, svg_dataset.py:139-140)"""
        self._gen = torch.Generator(device=self.device)
        self._gen.manual_seed(int(seed))
        return self

    # ---- the batch path -----------------------------------------------------------------------------------------
    def batch(self, icon_idx, model_args=None, random_aug=True, aug=None):
        """What DataLoader(default collate) over the reference's `get(i, model_args)` returns for the icons `icon_idx`, with
        ``preprocess`` applied on the way: {"commands": [N, G, S+2], "args": [N, G, S+2, 11], ...}, one launch per layout.
        `aug` (optional): an (N, 3) tensor of (dx, dy, factor) in the store's view box, one row per ITEM of the batch, pins
        the draws; otherwise random_aug draws them per item (`paths.augment_params`), and random_aug=False is
        ``preprocess(augment=False)``: the numericalize chain only."""
        st = self.store
        model_args = list(model_args if model_args is not None else self.model_args)
        icon = torch.as_tensor(icon_idx, dtype=torch.int64).to(self.device).reshape(-1) % st.n_icons
        N = icon.numel()
        variant = st.var_base[icon].to(torch.int32).contiguous()
        vb, n = st.viewbox, self.ARGS_DIM
        if aug is not None:
            aug = torch.as_tensor(aug, dtype=torch.float32).to(self.device)
            if tuple(aug.shape) != (N, 3):
                raise DsvgError(f"aug is (N, 3) = (dx, dy, factor) per item; got {tuple(aug.shape)} for {N} items")
            factor, vec = aug[:, 2], aug[:, :2]
        elif random_aug:
            factor, vec = paths.augment_params(N, viewbox=vb, generator=self._gen, device=self.device)
        augmented = aug is not None or random_aug
        kinds, base = self._chains[augmented]
        params = base.repeat(N, 1, 1)
        if augmented:                               # zoom(factor) = T(-c), S(factor), T(c); then T(vec)
            params[:, 1, 0] = factor
            params[:, 3, :2] = vec
        res = {}
        for grouped in (False, True):
            sfx = "_grouped" if grouped else ""
            keys = [k for k in ("commands", "args", "args_rel") if k + sfx in model_args]
            if not keys:
                continue
            L = (self.MAX_TOTAL_LEN if grouped else self.MAX_SEQ_LEN) + 2
            cmds, args, rel = ops.assemble_augmented(st.rows, st.slot_off, variant, st.G, L, grouped, kinds, params,
                                                     numericalize=n, want_args="args" in keys,
                                                     want_rel="args_rel" in keys, pad_val=float(self.PAD_VAL), args_dim=n)
            for k, v in (("commands", cmds), ("args", args), ("args_rel", rel)):
                if k in keys:
                    res[k + sfx] = v
        unknown = [k for k in model_args if k not in res and k not in ("filling", "label")]
        if unknown:
            raise DsvgError(f"model_args {unknown} are not produced by the device batch assembly")
        if "filling" in model_args:
            res["filling"] = st.filling[icon].unsqueeze(-1)         # (N, G, 1) int64, svg_dataset.py:209-210
        if "label" in model_args:
            if st.label is None:
                raise DsvgError("the store has no labels")
            res["label"] = st.label[icon]
        return res

    # ---- per-item surface of the reference ------------------------------------------------------------------------
    def get(self, idx=0, model_args=None, random_aug=True, id=None, svg=None):
        """svg_dataset.py:158-172 (without the `svg=` path): per-item tensors, e.g. commands [G, S+2]"""
        if svg is not None:
            raise NotImplementedError("get(svg=...) takes a drawing object of the reference's svglib; pack its tensors "
                                      "into a PackedSVGStore(numericalized=False) instead")
        if id is not None:
            idx = self.store.ids.index(id)
        out = self.batch([idx], model_args, random_aug)
        return {k: v[0] for k, v in out.items()}

    def __getitem__(self, idx):
        if self.deferred:
            return _Deferred(self, int(idx))
        return self.get(idx, self.model_args)

    def random_icon(self):
        return self.get(int(torch.randint(0, len(self), (1,))))


def load_dataset(cfg):
    """deepsvg/svg_dataset.py:218-222 over a saved float32 store: cfg.data_dir is the store file, or a directory that holds
    svg_store.npz (`PackedSVGStore.save`)"""
    path = cfg.data_dir if os.path.isfile(cfg.data_dir) else os.path.join(cfg.data_dir, STORE_FILE)
    return SVGDataset(store=PackedSVGStore.load(path), model_args=cfg.model_args, max_num_groups=cfg.max_num_groups,
                      max_seq_len=cfg.max_seq_len, max_total_len=cfg.max_total_len,
                      nb_augmentations=getattr(cfg, "nb_augmentations", 1),
                      deferred=getattr(cfg, "collate_fn", None) is device_collate, device=getattr(cfg, "device", "cuda"))
