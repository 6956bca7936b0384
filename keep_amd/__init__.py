"""keep_amd: MI355X (gfx950) native zero-shot WSI inference engine for the KEEP hot path.

Public surface mirrors the reference model API (quick_start/keep_inference.py:25-73):

    from keep_amd import KEEPModel
    model = KEEPModel.from_pretrained(release_dir).to("cuda").eval()
    img = model.encode_image(tiles)          # [B,768] unit-norm fp32
    txt = model.encode_text(token_inputs)    # [P,768] unit-norm fp32
    sim = img @ txt.T                        # or model.similarity(img, txt, mode=...)
"""
from .config import KEEPShape, TextShape, VisionShape, bert_flops_per_prompt, vit_flops_per_tile
from .model import KEEPModel, PROFILE_TAGS

__all__ = ["KEEPModel", "KEEPShape", "VisionShape", "TextShape", "PROFILE_TAGS",
           "vit_flops_per_tile", "bert_flops_per_prompt"]
from .lesion import FrocAccumulator, FrocCurve, camelyon16_margin
from .morphometry import RegionShape, camelyon16_itc_axis

__all__ += ["FrocAccumulator", "FrocCurve", "camelyon16_margin", "RegionShape", "camelyon16_itc_axis"]
from .bootstrap import BootstrapResult

__all__ += ["BootstrapResult"]
from .stain import StainFit, StainTarget

__all__ += ["StainFit", "StainTarget"]
from .quality import QualityGate, QualityRules, TileQuality

__all__ += ["QualityGate", "QualityRules", "TileQuality"]
__version__ = "0.1.0"
