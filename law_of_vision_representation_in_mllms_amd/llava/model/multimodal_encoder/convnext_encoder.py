"""ConvNextVisionTower on MI355X - HF ConvNextModel / OpenCLIP's timm ConvNeXt trunks behind the reference's tower protocol.

Not in the reference registry: users add the checkpoint id or directory to llava_arch.build_function_mapping with
builder.build_convnext_vision_tower.  A ConvNeXt has five hidden states - the stem output and the four stage outputs - and no class token:
`select_layer` indexes those five (negative values from the end, -1 = the stride-32 map, -2 = the stride-16 map), `select_feature` is 'patch'
only, `hidden_size` and `num_patches` are those of the selected state.  `vit_img_size` re-targets the input side (any multiple of 32)."""
from __future__ import annotations

from types import SimpleNamespace

from .... import convnext_weights as CW
from ._vit_tower import PatchMapTower, _processor_crop
from .image_processing import OPENAI_CLIP_MEAN, OPENAI_CLIP_STD


class ConvNextVisionTower(PatchMapTower):
    FAMILY = "convnext"
    WEIGHTS, ENGINE = CW, "make_convnext_engine"
    MEAN, STD = OPENAI_CLIP_MEAN, OPENAI_CLIP_STD           # the OpenCLIP statistics

    def __init__(self, vision_tower, args, delay_load=False):
        self._require_patch(getattr(args, "mm_vision_select_feature", self.DEFAULT_SELECT_FEATURE))      # the first error, as everywhere
        if not -5 <= args.mm_vision_select_layer <= 4:
            raise ValueError(f"select_layer {args.mm_vision_select_layer} is outside the five hidden states of a ConvNeXt (0 = stem, 1 .. 4 = stages)")
        super().__init__(vision_tower, args, delay_load=delay_load)

    def _hf_spec(self, cfg, path):
        return CW.spec_from_hf_config(cfg, self.vision_tower_name, crop_size=_processor_crop(path))

    def _retarget(self, spec):                               # a fully convolutional tower: no table to resize
        return spec.at_resolution(int(self._img_size)) if self._img_size and self._img_size != spec.image_size else spec

    def _state(self):
        return self.select_layer if self.select_layer >= 0 else 5 + self.select_layer

    def _config_for(self, spec):
        k = self._state()
        # patch_size: the selected state's stride, so that the protocol's (image_size // patch_size) ** 2 is its token count
        return SimpleNamespace(hidden_size=spec.width(k), image_size=spec.image_size, patch_size=spec.image_size // spec.grid(k),
                               hidden_sizes=list(spec.hidden_sizes), depths=list(spec.depths), num_hidden_layers=4)
