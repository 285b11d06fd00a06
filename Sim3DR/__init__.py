"""Drop-in for the reference's `Sim3DR` package (`from Sim3DR import RenderPipeline`, `get_normal`, `rasterize`,
`rasterize_triangles`, `render_texture_core`): the same names,
served by the HIP kernels of synergynet_amd (no Cython extension to build)."""
from synergynet_amd.sim3dr import RenderPipeline, get_normal, rasterize, rasterize_triangles, render_texture_core  # noqa: F401
