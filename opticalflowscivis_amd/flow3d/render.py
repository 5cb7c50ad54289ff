"""Pictures of volumes with the Flow-3D tools: `python -m opticalflowscivis_amd.flow3d.render --seq frames.npy --tf hot
--range 0 1 --image 512 512 --azimuth 30 --elevation 20 --orbit 3 --out img.npy --png-dir shots --json r.json` ray-casts
every frame (or every step of a --field that ftle, vortex or regions wrote) on the device; see
opticalflowscivis_amd/render.py."""
from ..render import main3d

if __name__ == "__main__":
    main3d()
