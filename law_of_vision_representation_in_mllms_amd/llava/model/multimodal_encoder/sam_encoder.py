"""SamVisionTower on MI355X - HF SamVisionModel (the Segment Anything image encoder) behind the reference's tower protocol.

Not in the reference registry: users add the checkpoint id or directory to llava_arch.build_function_mapping with
builder.build_sam_vision_tower.  The tower has L + 2 states and no class token: the L + 1 hidden states of the ViT (index 0 = patch embedding
+ positions) as [B, g g, d] and then the neck map [B, g g, 256]; `select_layer` indexes those (-1 = the neck map, what the MLLMs that carry a
SAM branch consume; -2 = the last block), `select_feature` is 'patch' only, `hidden_size` and `num_patches` are those of the selected state.
The input side cannot be re-targeted (`vit_img_size` other than the checkpoint's is an error, as in the reference module)."""
from __future__ import annotations

from types import SimpleNamespace

from .... import sam_weights as SW
from ._vit_tower import PatchMapTower


class SamVisionTower(PatchMapTower):
    FAMILY = "sam"
    WEIGHTS, ENGINE = SW, "make_sam_engine"
    MEAN, STD = SW.SAM_MEAN, SW.SAM_STD                      # SAM's published statistics

    def _hf_spec(self, cfg, path):
        return SW.spec_from_hf_config(cfg, self.vision_tower_name, vit_img_size=self._img_size or None)

    def _spec(self, path):
        spec = super()._spec(path)
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
