"""Converts the per-vertex positions and normals of the reference's models/lagergehaeuse.ply (ASCII PLY, 14136 vertices,
BSD-licensed) into tests/golden/lagergehaeuse_normals.npz: the model cloud of the ICP refinement (loadPLYSimple(path, 1)).
Run in the build container only (needs /root/reference)."""
import os
import numpy as np

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
lines = open(os.path.join(REF, "models", "lagergehaeuse.ply")).read().split("\n")
nv = int([l for l in lines if l.startswith("element vertex")][0].split()[-1])
h = lines.index("end_header") + 1
xyzn = np.array([[float(t) for t in l.split()[:6]] for l in lines[h:h + nv]], np.float32)
assert xyzn.shape == (14136, 6)
np.savez_compressed(os.path.join(HERE, "lagergehaeuse_normals.npz"), xyzn=xyzn)
print("vertices with normals:", xyzn.shape)
