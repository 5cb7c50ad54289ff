"""Meshes of volumes with the Flow-3D tools: `python -m opticalflowscivis_amd.flow3d.isosurface --seq frames.npy --iso 0.5
--mesh-dir meshes --format ply --json r.json` extracts the surface f = iso of every frame (or of every step of a --field
that ftle, vortex or regions wrote, coloured by a --color-field) on the device; see opticalflowscivis_amd/isosurface.py."""
from ..isosurface import main3d

if __name__ == "__main__":
    main3d()
