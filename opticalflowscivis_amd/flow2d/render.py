"""Pictures of 2-D frames and fields with the Flow-2D tools: `python -m opticalflowscivis_amd.flow2d.render --seq
frames.npy --tf grey --flows flows.npy --png-dir shots --json r.json` colour-maps every frame (or every step of a
--field) through the transfer function and writes flow2rgb pictures of --flows; see opticalflowscivis_amd/render.py."""
from ..render import main2d

if __name__ == "__main__":
    main2d()
