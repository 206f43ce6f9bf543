"""Scene file I/O of the reference's ``datasets`` package (inference side)."""
from .dataset_reader_physics import (Dataset, DatasetGroup, PhysicsSimDataFlow, get_dataloader, get_rollout,  # noqa: F401
                                     read_scene, write_results,
                                     write_results_npz, write_scene)
