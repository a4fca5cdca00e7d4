"""ConvNextVisionTower on MI355X - HF ConvNextModel / OpenCLIP's timm ConvNeXt trunks behind the reference's tower protocol.

Not in the reference registry: users add the checkpoint id or directory to llava_arch.build_function_mapping with
builder.build_convnext_vision_tower.  A ConvNeXt has five hidden states - the stem output and the four stage outputs - and no class token:
`select_layer` indexes those five (negative values from the end, -1 = the stride-32 map, -2 = the stride-16 map), `select_feature` is 'patch'
only, `hidden_size` and `num_patches` are those of the selected state.  `vit_img_size` re-targets the input side (any multiple of 32)."""
from __future__ import annotations

import json
import os
from types import SimpleNamespace

import torch

from .... import convnext_weights as CW
from ._vit_tower import HipViTTower, _EngineModule, _find_local_checkpoint, _load_state_dict, _processor_crop
from .image_processing import OPENAI_CLIP_MEAN, OPENAI_CLIP_STD, SimpleImageProcessor


class ConvNextVisionTower(HipViTTower):
    FAMILY = "convnext"
    DEFAULT_SELECT_FEATURE = "patch"

    def __init__(self, vision_tower, args, delay_load=False):
        feature = getattr(args, "mm_vision_select_feature", self.DEFAULT_SELECT_FEATURE)
        if feature != "patch":                               # the protocol's error, before anything is loaded: there is no class token to keep
            raise ValueError(f"Unexpected select feature: {feature}")
        if not -5 <= args.mm_vision_select_layer <= 4:
            raise ValueError(f"select_layer {args.mm_vision_select_layer} is outside the five hidden states of a ConvNeXt (0 = stem, 1 .. 4 = stages)")
        super().__init__(vision_tower, args, delay_load=delay_load)

    # ------------------------------------------------------------------ loading
    def _spec(self, path):
        if path is not None:
            from transformers import AutoConfig
            return CW.spec_from_hf_config(AutoConfig.from_pretrained(path), self.vision_tower_name, crop_size=_processor_crop(path))
        if self.vision_tower_name in CW.SPECS:
            return CW.SPECS[self.vision_tower_name]
        raise OSError(f"{self.vision_tower_name} is not a local checkpoint directory, is not in the offline HF cache and has no built-in architecture")

    def _retarget(self, spec):
        return spec.at_resolution(int(self._img_size)) if self._img_size and self._img_size != spec.image_size else spec

    def _state(self):
        return self.select_layer if self.select_layer >= 0 else 5 + self.select_layer

    def _config_for(self, spec):
        k = self._state()
        # patch_size: the selected state's stride, so that the protocol's (image_size // patch_size) ** 2 is its token count
        return SimpleNamespace(hidden_size=spec.width(k), image_size=spec.image_size, patch_size=spec.image_size // spec.grid(k),
                               hidden_sizes=list(spec.hidden_sizes), depths=list(spec.depths), num_hidden_layers=4)

    def _config_only(self):
        return self._config_for(self._retarget(self._spec(_find_local_checkpoint(self.vision_tower_name))))

    def _make_image_processor(self, spec, path=None):
        """preprocessor_config.json when the directory has one (mean / std; the sizes follow the tower's input side), else resize + centre crop to
        the spec size with the OpenCLIP statistics."""
        mean, std = OPENAI_CLIP_MEAN, OPENAI_CLIP_STD
        f = os.path.join(path, "preprocessor_config.json") if path else None
        if f and os.path.exists(f):
            with open(f) as fh:
                pc = json.load(fh)
            mean, std = tuple(pc.get("image_mean", mean)), tuple(pc.get("image_std", std))
        return SimpleImageProcessor(spec.image_size, spec.image_size, mean, std)

    def load_model(self):
        from .... import engine
        path = _find_local_checkpoint(self.vision_tower_name)
        spec = self._spec(path)
        if path is not None:
            w = CW.pack_hf_state_dict(_load_state_dict(path), spec)
        elif self._synthetic:
            w = CW.synthetic_weights(spec, seed=1)
        else:
            raise OSError(f"{self.vision_tower_name} is not a local checkpoint directory and is not in the offline HF cache "
                          "(set VISREP_SYNTHETIC_WEIGHTS=1 or args.synthetic_weights for deterministic random-init weights)")
        spec = self._retarget(spec)                          # a fully convolutional tower: no table to resize
        self.spec = spec
        self.image_processor = self._make_image_processor(spec, path)
        eng = engine.make_convnext_engine(spec, w, self._device, "fp32" if self._precision in ("fp32", "float32") else self._precision)
        self.vision_tower = _EngineModule(eng, self._config_for(spec), torch.bfloat16)
        self.vision_tower.requires_grad_(False)
        self.is_loaded = True

    def feature_select(self, image_forward_outs):
        if self.select_feature != "patch":
            raise ValueError(f"Unexpected select feature: {self.select_feature}")
        return image_forward_outs.hidden_states[self.select_layer]       # every row is a patch: nothing to drop
