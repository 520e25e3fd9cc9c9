"""Import-name shim: ``sdf_sampler.sdf_sampler`` re-exports deepsdf_amd/sdf_sampler.py (the reference module's API)."""
from deepsdf_amd.sdf_sampler import (BoxSDF, DataSetInfo, NegatedCallable, RandomSampleSDF, SDFBase, SDFfromMesh,  # noqa: F401
                                     SDFSampler, SphereParameters, SummedSDF, random_points_cube, random_sample_sdf)
