"""SamVisionTower on MI355X - HF SamVisionModel (the Segment Anything image encoder) behind the reference's tower protocol.

Not in the reference registry: users add the checkpoint id or directory to llava_arch.build_function_mapping with
builder.build_sam_vision_tower.  The tower has L + 2 states and no class token: the L + 1 hidden states of the ViT (index 0 = patch embedding
+ positions) as [B, g g, d] and then the neck map [B, g g, 256]; `select_layer` indexes those (-1 = the neck map, what the MLLMs that carry a
SAM branch consume; -2 = the last block), `select_feature` is 'patch' only, `hidden_size` and `num_patches` are those of the selected state.
The input side cannot be re-targeted (`vit_img_size` other than the checkpoint's is an error, as in the reference module)."""
from __future__ import annotations

import json
import os
from types import SimpleNamespace

import torch

from .... import sam_weights as SW
from ._vit_tower import HipViTTower, _EngineModule, _find_local_checkpoint, _load_state_dict
from .image_processing import SimpleImageProcessor


class SamVisionTower(HipViTTower):
    FAMILY = "sam"
    DEFAULT_SELECT_FEATURE = "patch"

    def __init__(self, vision_tower, args, delay_load=False):
        feature = getattr(args, "mm_vision_select_feature", self.DEFAULT_SELECT_FEATURE)
        if feature != "patch":                               # the protocol's error, before anything is loaded: there is no class token to keep
            raise ValueError(f"Unexpected select feature: {feature}")
        super().__init__(vision_tower, args, delay_load=delay_load)

    # ------------------------------------------------------------------ loading
    def _spec(self, path):
        if path is not None:
            from transformers import AutoConfig
            spec = SW.spec_from_hf_config(AutoConfig.from_pretrained(path), self.vision_tower_name, vit_img_size=self._img_size or None)
        elif self.vision_tower_name in SW.SPECS:
            spec = SW.SPECS[self.vision_tower_name]
        else:
            raise OSError(f"{self.vision_tower_name} is not a local checkpoint directory, is not in the offline HF cache and has no built-in architecture")
        if self._img_size and int(self._img_size) != spec.image_size:
            raise ValueError(f"SAM: vit_img_size {self._img_size} differs from the tower's image_size {spec.image_size}: the input side cannot be re-targeted")
        if not -spec.n_states <= self.select_layer < spec.n_states:
            raise ValueError(f"select_layer {self.select_layer} is outside the {spec.n_states} states of this SAM tower")
        return spec

    def _state(self, spec):
        return self.select_layer if self.select_layer >= 0 else spec.n_states + self.select_layer

    def _config_for(self, spec):
        return SimpleNamespace(hidden_size=spec.width(self._state(spec)), image_size=spec.image_size, patch_size=spec.patch,
                               num_hidden_layers=spec.layers + 1, output_channels=spec.out_channels)

    def _config_only(self):
        return self._config_for(self._spec(_find_local_checkpoint(self.vision_tower_name)))

    def _make_image_processor(self, spec, path=None):
        """Resize to the spec side with the checkpoint's mean / std when the directory has a preprocessor_config.json, else SAM's published ones."""
        mean, std = SW.SAM_MEAN, SW.SAM_STD
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
            w = SW.pack_hf_state_dict(_load_state_dict(path), spec)
        elif self._synthetic:
            w = SW.synthetic_weights(spec, seed=1)
        else:
            raise OSError(f"{self.vision_tower_name} is not a local checkpoint directory and is not in the offline HF cache "
                          "(set VISREP_SYNTHETIC_WEIGHTS=1 or args.synthetic_weights for deterministic random-init weights)")
        self.spec = spec
        self.image_processor = self._make_image_processor(spec, path)
        eng = engine.make_sam_engine(spec, w, self._device, "fp32" if self._precision in ("fp32", "float32") else self._precision)
        self.vision_tower = _EngineModule(eng, self._config_for(spec), torch.bfloat16)
        self.vision_tower.requires_grad_(False)
        self.is_loaded = True

    def feature_select(self, image_forward_outs):
        if self.select_feature != "patch":
            raise ValueError(f"Unexpected select feature: {self.select_feature}")
        return image_forward_outs.hidden_states[self.select_layer]       # every row is a patch: nothing to drop
