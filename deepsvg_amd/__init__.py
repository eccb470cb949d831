"""deepsvg_amd — MI355X (gfx950) native implementation of the DeepSVG SVGTransformer train/infer hot path.

Public surface mirrors the reference (alexandre01/deepsvg):
    deepsvg_amd.SVGTransformer  <->  deepsvg.model.model.SVGTransformer
    deepsvg_amd.SVGLoss         <->  deepsvg.model.loss.SVGLoss
    deepsvg_amd.config.*        <->  deepsvg.model.config.*
    deepsvg_amd.metrics         <->  deepsvg.difflib: SVGTensor.sample_points + chamfer_loss (reconstruction error)
                                     and the other losses of difflib/loss.py: svg_emd_loss, svg_length_loss, continuity_loss
    deepsvg_amd.render          <->  deepsvg.svglib: SVG.draw of a decoded batch (stroke / fill coverage images, interpolation)
    deepsvg_amd.paths           <->  deepsvg.svglib: SVG.canonicalize + numericalize of a batch (the form the encoder was trained on),
                                     its preprocessing chain, and SVG.zoom / rotate / translate / normalize
    deepsvg_amd.svgio           <->  deepsvg.svglib: SVG.load_svg of a batch of documents (path text parsed on the device), the
                                     dataset/preprocess.py chain over files, and the way back out as SVG text
    deepsvg_amd.dataset         <->  deepsvg.svgtensor_dataset (stored augmentations); deepsvg_amd.svg_dataset <-> deepsvg.svg_dataset
                                     (augmentation on the fly); both imported by name, as cfg.dataloader_module
"""
# (No process-wide side effects on import.  The data-parallel hipGraph step wants GPU_MAX_HW_QUEUES=6 in the environment BEFORE
# the HIP runtime comes up - see trainer.HW_QUEUES_NOTE; bench.py sets it, TrainStep warns when a data-parallel trainer
# finds it unset.)

from .config import _DefaultConfig, Hierarchical, HierarchicalOrdered, OneStageOneShot  # noqa: F401
from .model import SVGTransformer  # noqa: F401
from .loss import SVGLoss  # noqa: F401
from . import metrics  # noqa: F401
from . import render  # noqa: F401
from . import paths  # noqa: F401
from . import svgio  # noqa: F401

__all__ = ["SVGTransformer", "SVGLoss", "_DefaultConfig", "Hierarchical", "HierarchicalOrdered", "OneStageOneShot", "metrics",
           "render", "paths", "svgio"]
