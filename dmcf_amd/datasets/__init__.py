"""The reference's ``datasets`` package: scene file I/O, the data flow, and the column / free-fall generators."""
from .dataset_reader_physics import (Dataset, DatasetGroup, PhysicsSimDataFlow, get_dataloader, get_rollout,  # noqa: F401
                                     read_scene, write_results,
                                     write_results_npz, write_scene)
