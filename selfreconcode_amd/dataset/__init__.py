from .dataset import (ClipSampler, FrameLoader, RandomSampler, SceneDataset, getDatasetAndLoader, make_conds,  # noqa: F401
                      read_scene_folder)
