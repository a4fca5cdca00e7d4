"""InternViTVisionTower on MI355X - the vision tower of the InternVL family (HF InternVLVisionModel) behind the reference's tower protocol.

Not in the reference registry: users add the checkpoint id or directory to llava_arch.build_function_mapping with
builder.build_internvit_vision_tower.  The checkpoint directory is a transformers-layout InternVL checkpoint (its `vision_config` and the
`vision_tower.` weights are taken) or a bare InternVLVisionModel.  InternVL's pixel-shuffle projector is not part of the tower."""
from ._vit_tower import HipViTTower


class InternViTVisionTower(HipViTTower):
    FAMILY = "internvl"
    DEFAULT_SELECT_FEATURE = "patch"

    def __init__(self, vision_tower, args, delay_load=False):
        super().__init__(vision_tower, args, delay_load=delay_load)
        if delay_load:
            return
        self.cfg_only = self.config
