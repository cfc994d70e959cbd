"""`python -m firework_amd` — the reference's command line (src/main.rs:6-62) on the HIP path.

    firework --scene-file <yml> -s <samples> [-n <name>] [-o <png>]

Same fixed view as main.rs: camera (0,30,50) -> (0,0,0), fov 40, 960x540, use_bvh(true); prints
`Finished Rendering in {} s`.  Without `-o` the reference opens a minifb window; a GPU node has no display,
so `-o` is required here.  Extra flags (not in the reference): --width/--height/--seed/--device, and
--progressive N (write the image after each of N passes) / --checkpoint FILE (save the accumulation buffer after every
pass and resume from it: the finished image is bit-identical to an uninterrupted render), --adaptive TOL [--min-samples M]
(adaptive sampling up to -s samples per pixel; not with --progressive / --checkpoint), --orbit N (a turntable: N views evenly spaced
in azimuth around the fixed camera's look-at point, rendered in one call; -o must hold a format field, e.g. 'frame_{:03d}.png', which
receives the view number; not with --progressive / --checkpoint / --adaptive), --denoise [L] (filter the frame with L a-trous
iterations, default 5, guided by first-hit albedo / normal / position buffers; with a plain render or --adaptive, whose moments and
per-pixel counts it uses; not with --progressive / --checkpoint / --orbit), --camera {pinhole,panorama,orthographic} (default pinhole:
the fixed view above; panorama: an equirectangular 360-degree image from the fixed camera's position, --width x --height, which loads
back as an HDR environment with the same orientation; orthographic: the fixed view's direction with parallel rays over a view plane
--ortho-height H high, by default the height the fixed view sees at its look-at point; both rendered through caller-supplied rays, not
with --orbit / --adaptive / --denoise / --progressive / --checkpoint), --light-sampling (sample the lights directly at diffuse vertices:
next-event estimation with MIS; combines with every other flag), --env-sampling (sample an HDR environment map by its
radiance at diffuse vertices; alone or with --light-sampling, and with every other flag), --all-emitters (light sampling
over every emitting primitive, meshes, disks and boxes included, picked by power; implies --light-sampling),
--temporal [MAX_HISTORY] (only with --orbit: the views are rendered one after another as a sequence, each merged with the reprojected
history of the view before it — a pixel carries over at most MAX_HISTORY samples, default 64 — and then denoised, DESIGN.md §9j;
--denoise L and --aov-samples keep their meaning; view k renders with seed + k; not with --progressive / --checkpoint / --adaptive /
--camera), --camera fisheye [--fisheye-fov DEG] (an equidistant full-frame fisheye along the fixed view's direction, DEG degrees across
the image diagonal, default 180; combines as the other models do).  The three models' rays are generated on the device
(fw_render_model).  --bake-probes NX,NY,NZ --probe-min x,y,z --probe-max x,y,z [--probe-dirs D] [--probe-rounds R]
(no image: a grid of irradiance probes between the two corners, D directions each, default 256, R rounds of -s samples per direction,
default 1, baked on the device into nine SH coefficients per probe and channel, fw_bake_probes; -o names an .npz with
positions, sh, sums, rounds, directions and samples; --light-sampling, --env-sampling and --all-emitters apply; not with --camera /
--denoise / --orbit / --adaptive / --progressive / --checkpoint / --temporal).  --bake-lightmap OBJECT,W,H [--lightmap-dirs D]
[--lightmap-rounds R] [--lightmap-dilate N] (no image: the irradiance over the W x H UV texels of render object OBJECT, which must be
a triangle mesh with uvs, D cosine-weighted directions per texel, default 64, R rounds of -s samples per direction, default 1, N
dilation passes over the seams, default 2, baked on the device, fw_bake_lightmap; -o names an .npz with irradiance,
sums, owner, rounds, directions and samples; the sampling flags apply; refuses what --bake-probes refuses, and --bake-probes).
--probe-lit PROBES.npz [--probe-no-wrap] (a preview of the fixed view lit from the probes a --bake-probes run saved: one first-hit pass
of --aov-samples samples and no paths, direct and indirect diffuse light both looked up in the grid, fw_probe_shade; the
file must hold sh, grid_lo, grid_hi and grid_counts; --probe-no-wrap turns the guard against probes behind the surface off; -s is
not used; refuses what --bake-probes refuses, --bake-probes and --bake-lightmap).  --bake-probes ... --probe-depth R
[--probe-depth-sharpness K] [--probe-depth-max M] (also bakes every probe's R x R octahedral map of depth moments, R in 4, 8, 16, 32,
weights cos^(2^K), K in 0..8, default 6, distances clamped to M, default the grid's diagonal, over the same --probe-rounds rounds,
fw_bake_probe_depth; the .npz also gets depth, depth_res, depth_sharpness and depth_max).  --probe-lit then weights every
probe by its visibility from the surface (fw_probe_shade_vis) when the file holds them; --probe-no-visibility ignores them (the image
of a file without them), --probe-normal-bias B moves the looked-up point B >= 0 world units along its normal first (default 0).
--bake-probes ... --probe-relocate MIN_FRONT [--probe-relocate-steps K] [--probe-relocate-max F] (first moves probes out of geometry and
marks those that stay inside inactive, fw_relocate_probes, DESIGN.md §9u: K moving steps, default 4, no offset beyond F, default 0.45,
of the grid's spacing; sh and depth are baked at the moved positions; the .npz keeps the nominal positions and also gets placement,
relocate_min_front and relocate_steps).  --probe-lit then reads the probes where they went (fw_probe_shade_placed) when the file holds
placement; --probe-no-placement ignores it.
--bake-probes ... --probe-radiance R [--probe-radiance-sharpness K] [--probe-radiance-roughness a,b,...] (also bakes every probe's R x R
octahedral radiance map and its GGX-prefiltered level chain, R in 4, 8, 16, 32, level 0's weights cos^(2^K), default K = 2, one level
per roughness, default 0.1 .. 1 over as many levels as fit, fw_bake_probe_radiance, DESIGN.md §9v: one render pass feeds the SH and
the maps; the .npz also gets radiance, radiance_res, radiance_sharpness and radiance_roughness).  --probe-lit then shows reflections on
GgxMat and MetalMat surfaces (fw_probe_shade_glossy) when the file holds them; --probe-no-radiance ignores them.
--ao RADIUS [--ao-dirs D] [--ao-rounds R] [--ao-falloff] (the fixed view's ambient occlusion as a grey PNG: one first-hit pass of
--aov-samples samples, then R rounds, default 1, of D cosine-weighted rays per pixel, default 64, traced from each pixel's surface point;
a hit nearer than RADIUS > 0 occludes, fully or with --ao-falloff by 1 - dist / RADIUS, fw_bake_ao; -s is not used;
refuses what --probe-lit refuses, and --probe-lit).  --bake-lightmap ... --lightmap-ao RADIUS (also bakes the occlusion over the same
texels with the same --lightmap-dirs, --lightmap-rounds and --lightmap-dilate; --ao-falloff applies; the .npz also gets ao and bent).
--direct-light [--direct-bias B] (the fixed view lit by the scene's point, spot and directional lights alone: one first-hit pass of
--aov-samples samples, then one shadow ray per pixel and light, origins moved B >= 0, default 0.001, along the normal: sharp shadows and
GgxMat highlights without a path, fw_bake_direct; -s is not used; refuses what --ao refuses, and --ao).  --probe-lit FILE
--direct-light (adds that light, which no probe holds, to the probe-lit frame).  --bake-lightmap ... --lightmap-direct [--direct-bias B]
(adds the lights' irradiance at each covered texel before the dilation; the .npz also gets direct).
--sun-sky EL,AZ[,TURBIDITY] [--sun-sky-size W,H] [--sun disc|light|none] (replaces the scene's environment by an analytic sun and sky,
the sun EL degrees above the horizon at azimuth AZ degrees, baked on the device into a W x H map, default 2048,1024, fw_sky_map,
DESIGN.md §9x; the sun is a disc in the map, the default, which --env-sampling finds; or a directional light of the same energy beside
a map without it, which --light-sampling and --direct-light find; or absent; --sun light refuses --env-sampling; combines with every
other flag).
--probe-lit FILE --probe-split-sum [N_MU,N_RHO] [--probe-energy] (shades GgxMat and MetalMat pixels with the split sum's BRDF term,
F0 A + B from an N_MU x N_RHO table of the GGX directional albedo, default 64,64, each in 2..256, baked on the device in the call,
fw_ggx_table and fw_probe_shade_split, DESIGN.md §9y, in the place of the bare Schlick term: a rough conductor is no longer several
times too bright; --probe-energy also multiplies by 1 + F0 (1 / (A + B) - 1), the single-lobe energy compensation; both need a file
that holds radiance maps and refuse --probe-no-radiance).
--probe-lit FILE --probe-gather D[,ROUNDS] [--gather-bias B] (a final gather: the probes are read one bounce away, at the hits of D
cosine-weighted gather rays per pixel and round, default 1 round, origins moved B >= 0, default 0.001, along the normal; a ray that hits
an emitter brings its emission, one that misses the environment: contact shadows, near-field colour bleeding and directly seen emitters
from the same probes file, fw_bake_gather; with --direct-light the lights are added at the gather hits as well; refuses
--ao, --probe-split-sum and a file's radiance maps in use: pass --probe-no-radiance).
--probe-lit FILE --probe-reflect D[,ROUNDS] [--reflect-bias B] (traced reflections on GgxMat and MetalMat pixels: D reflection rays per
glossy pixel and round, default 1 round, drawn from the GGX lobe around the view direction, origins moved B >= 0, default 0.001, along
the normal, lit at their hits as gather rays are and summed with the weight F G2 / G1: parallax-correct reflections with the split sum's
BRDF term and no radiance maps, fw_bake_reflect; every other pixel is shaded as without the flag, --probe-gather
included; with --direct-light the lights are added at the reflection rays' hits as well; refuses --ao, --probe-split-sum and a file's
radiance maps in use: pass --probe-no-radiance).
--area-light S[,ROUNDS] [--area-bias B] (the fixed view lit by the scene's sampled area lights alone, every EmissiveMat sphere and
axis-aligned rectangle: one first-hit pass of --aov-samples samples, then S shadow rays per pixel, light and round, default 1 round,
towards points drawn on the light as the pixel sees it, origins moved B >= 0, default 0.001, along the normal: soft shadows without a
path, fw_bake_area; -s is not used; refuses what --direct-light refuses, and --direct-light).  --probe-lit FILE
--probe-gather D --area-light S (the final-gather split: the gather rays bring back nothing from those lights, FW_GATHER_NO_LIGHTS, and
the lights' sampled irradiance is added to the gathered one before shading).  --probe-lit FILE --area-light S without --probe-gather is
an error: the probes already hold the emitters' direct light, and adding it would count it twice.
--emitter-light S[,ROUNDS] [--emitter-bias B] (the same three behaviours over every emitter of the scene — spheres, rectangles, Rect3d
faces, disks and mesh triangles: S shadow rays per pixel and round whatever the number of emitters, each towards an emitter picked in
proportion to area x power, fw_bake_emitters; alone the view lit by the emitters alone; with --probe-lit FILE
--probe-gather D the split with FW_GATHER_NO_EMITTERS; with --probe-lit alone an error; refuses what --area-light refuses, and
--area-light)."""
import argparse
import sys
import time


TEMPORAL_DEFAULT = 64.0    # api.DEFAULT_MAX_HISTORY (not imported here: the parser runs before the library is loaded)


def main(argv=None):
    ap = argparse.ArgumentParser(prog="firework")
    ap.add_argument("--scene-file", required=True)
    ap.add_argument("-n", "--name", default=None)
    ap.add_argument("-s", "--samples", type=int, required=True)
    ap.add_argument("-o", "--output", default=None)
    ap.add_argument("--width", type=int, default=960)
    ap.add_argument("--height", type=int, default=540)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--progressive", type=int, default=0, metavar="N", help="render in N passes, saving the image after each")
    ap.add_argument("--checkpoint", default=None, metavar="FILE", help=".npz accumulation checkpoint: written after every pass, resumed from if present")
    ap.add_argument("--adaptive", type=float, default=None, metavar="TOL",
                    help="adaptive sampling: render each pixel until its standard error is at most TOL x its brightness (-s is the cap)")
    ap.add_argument("--min-samples", type=int, default=16, metavar="M", help="with --adaptive: the samples every pixel gets first")
    ap.add_argument("--orbit", type=int, default=0, metavar="N",
                    help="render N views around the look-at point in one call; -o must hold a {} field for the view number")
    ap.add_argument("--denoise", type=int, nargs="?", const=5, default=None, metavar="L",
                    help="denoise the frame with L a-trous iterations (default 5) guided by first-hit albedo / normal / position buffers")
    ap.add_argument("--aov-samples", type=int, default=8, metavar="S", help="with --denoise: samples per pixel of the guide buffers")
    ap.add_argument("--temporal", type=float, nargs="?", const=TEMPORAL_DEFAULT, default=None, metavar="MAX_HISTORY",
                    help="with --orbit: merge each view with the reprojected history of the view before it (at most MAX_HISTORY samples "
                         "carried over per pixel, default 64), then denoise it")
    ap.add_argument("--light-sampling", action="store_true",
                    help="sample the scene's lights directly at diffuse vertices (next-event estimation with MIS): less noise per sample")
    ap.add_argument("--env-sampling", action="store_true",
                    help="importance-sample an HDR environment map at diffuse vertices (with --light-sampling: beside the lights)")
    ap.add_argument("--all-emitters", action="store_true",
                    help="light sampling over every emitting primitive (meshes, disks, boxes too), picked by power; implies --light-sampling")
    ap.add_argument("--camera", choices=("pinhole", "panorama", "orthographic", "fisheye"), default="pinhole",
                    help="camera model: the fixed pinhole view (default), an equirectangular panorama from its position, an orthographic "
                         "view, or an equidistant fisheye")
    ap.add_argument("--ortho-height", type=float, default=None, metavar="H",
                    help="with --camera orthographic: the height of the view plane (default: what the pinhole view sees at its look-at point)")
    ap.add_argument("--fisheye-fov", type=float, default=None, metavar="DEG",
                    help="with --camera fisheye: the angle across the image diagonal in degrees, in (0, 360] (default 180)")
    ap.add_argument("--bake-probes", default=None, metavar="NX,NY,NZ",
                    help="bake a grid of irradiance probes (nine SH coefficients per probe and channel) into the .npz named by -o")
    ap.add_argument("--probe-min", default=None, metavar="X,Y,Z", help="with --bake-probes: the grid's first corner")
    ap.add_argument("--probe-max", default=None, metavar="X,Y,Z", help="with --bake-probes: the grid's last corner")
    ap.add_argument("--probe-dirs", type=int, default=None, metavar="D", help="with --bake-probes: directions per probe and round (default 256)")
    ap.add_argument("--probe-rounds", type=int, default=None, metavar="R", help="with --bake-probes: rounds of -s samples per direction (default 1)")
    ap.add_argument("--probe-depth", type=int, default=None, metavar="R",
                    help="with --bake-probes: also bake an R x R map of depth moments per probe (R in 4, 8, 16, 32), for --probe-lit's visibility")
    ap.add_argument("--probe-depth-sharpness", type=int, default=None, metavar="K", help="with --probe-depth: a ray weighs cos^(2^K) in a texel, 0..8 (default 6)")
    ap.add_argument("--probe-depth-max", type=float, default=None, metavar="M",
                    help="with --probe-depth: distances are clamped to M > 0, which a miss counts as (default: the grid's diagonal)")
    ap.add_argument("--probe-radiance", type=int, default=None, metavar="R",
                    help="with --bake-probes: also bake an R x R octahedral radiance map per probe with a GGX-prefiltered level chain "
                         "(R in 4, 8, 16, 32), for --probe-lit's reflections; one render pass feeds it and the SH")
    ap.add_argument("--probe-radiance-sharpness", type=int, default=None, metavar="K",
                    help="with --probe-radiance: a ray weighs cos^(2^K) in a texel of level 0, 0..8 (default 2)")
    ap.add_argument("--probe-radiance-roughness", default=None, metavar="A,B,...",
                    help="with --probe-radiance: the levels' roughness, ascending in [0, 1] (default: 0.1 .. 1 over as many levels as fit)")
    ap.add_argument("--probe-no-radiance", action="store_true", help="with --probe-lit: ignore the radiance maps in the file")
    ap.add_argument("--bake-lightmap", default=None, metavar="OBJECT,W,H",
                    help="bake the irradiance over the W x H UV texels of render object OBJECT (a mesh with uvs) into the .npz named by -o")
    ap.add_argument("--lightmap-dirs", type=int, default=None, metavar="D", help="with --bake-lightmap: directions per texel and round (default 64)")
    ap.add_argument("--lightmap-rounds", type=int, default=None, metavar="R", help="with --bake-lightmap: rounds of -s samples per direction (default 1)")
    ap.add_argument("--lightmap-dilate", type=int, default=None, metavar="N", help="with --bake-lightmap: dilation passes over the seams, 0..64 (default 2)")
    ap.add_argument("--probe-relocate", type=float, default=None, metavar="MIN_FRONT",
                    help="with --bake-probes: first move probes out of geometry (at least MIN_FRONT > 0 from the nearest front face) and mark "
                         "those that stay inside inactive; sh and depth are baked at the moved positions")
    ap.add_argument("--probe-relocate-steps", type=int, default=None, metavar="K", help="with --probe-relocate: moving steps before the classification (default 4)")
    ap.add_argument("--probe-relocate-max", type=float, default=None, metavar="F",
                    help="with --probe-relocate: the largest offset as a fraction F >= 0 of the grid's spacing per axis (default 0.45)")
    ap.add_argument("--probe-no-placement", action="store_true", help="with --probe-lit: ignore the placement in the file")
    ap.add_argument("--probe-lit", default=None, metavar="PROBES.npz",
                    help="render the view lit from the irradiance probes that a --bake-probes run saved, without tracing paths")
    ap.add_argument("--probe-no-wrap", action="store_true", help="with --probe-lit: no guard against light from probes behind the surface")
    ap.add_argument("--probe-no-visibility", action="store_true", help="with --probe-lit: ignore the depth moments in the file")
    ap.add_argument("--probe-normal-bias", type=float, default=None, metavar="B",
                    help="with --probe-lit and depth moments: look visibility up B >= 0 world units along the normal (default 0)")
    ap.add_argument("--ao", type=float, default=None, metavar="RADIUS",
                    help="render the view's ambient occlusion as a grey PNG: a hit nearer than RADIUS occludes; no paths are traced")
    ap.add_argument("--ao-dirs", type=int, default=None, metavar="D", help="with --ao: rays per pixel and round (default 64)")
    ap.add_argument("--ao-rounds", type=int, default=None, metavar="R", help="with --ao: rounds of D rays per pixel (default 1)")
    ap.add_argument("--ao-falloff", action="store_true", help="with --ao or --lightmap-ao: a hit occludes by 1 - dist / RADIUS, not fully")
    ap.add_argument("--lightmap-ao", type=float, default=None, metavar="RADIUS",
                    help="with --bake-lightmap: also bake ambient occlusion and bent normals over the texels into the .npz")
    ap.add_argument("--direct-light", action="store_true",
                    help="render the direct light of the scene's point, spot and directional lights; with --probe-lit: add it to that frame")
    ap.add_argument("--lightmap-direct", action="store_true",
                    help="with --bake-lightmap: add the direct irradiance of the scene's point, spot and directional lights to the texels")
    ap.add_argument("--direct-bias", type=float, default=None, metavar="B",
                    help="with --direct-light or --lightmap-direct: move shadow-ray origins B >= 0 world units along the normal (default 0.001)")
    ap.add_argument("--sun-sky", default=None, metavar="EL,AZ[,TURBIDITY]",
                    help="replace the scene's environment by an analytic sun and sky: the sun EL degrees above the horizon at azimuth AZ degrees")
    ap.add_argument("--sun-sky-size", default=None, metavar="W,H", help="with --sun-sky: the size of the baked map (default 2048,1024)")
    ap.add_argument("--sun", choices=("disc", "light", "none"), default=None,
                    help="with --sun-sky: the sun as a disc in the map (default), as a directional light beside it, or not at all")
    ap.add_argument("--probe-split-sum", nargs="?", const="64,64", default=None, metavar="N_MU,N_RHO",
                    help="with --probe-lit: shade glossy pixels with the split sum's BRDF term from an N_MU x N_RHO GGX albedo table (default 64,64)")
    ap.add_argument("--probe-energy", action="store_true", help="with --probe-split-sum: the single-lobe energy compensation")
    ap.add_argument("--probe-gather", default=None, metavar="D[,ROUNDS]",
                    help="with --probe-lit: read the probes one bounce away, at the hits of D gather rays per pixel and round (default 1 round)")
    ap.add_argument("--gather-bias", type=float, default=None, metavar="B",
                    help="with --probe-gather: move gather-ray origins B >= 0 world units along the normal (default 0.001)")
    ap.add_argument("--probe-reflect", default=None, metavar="D[,ROUNDS]",
                    help="with --probe-lit: trace D GGX-sampled reflection rays per glossy pixel and round (default 1 round), lit from the probes at their hits")
    ap.add_argument("--reflect-bias", type=float, default=None, metavar="B",
                    help="with --probe-reflect: move reflection-ray origins B >= 0 world units along the normal (default 0.001)")
    ap.add_argument("--area-light", default=None, metavar="S[,ROUNDS]",
                    help="render the direct light of the scene's sphere and rectangle emitters, S shadow rays per pixel, light and round "
                         "(default 1 round); with --probe-lit and --probe-gather: the final-gather split")
    ap.add_argument("--area-bias", type=float, default=None, metavar="B",
                    help="with --area-light: move shadow-ray origins B >= 0 world units along the normal (default 0.001)")
    ap.add_argument("--emitter-light", default=None, metavar="S[,ROUNDS]",
                    help="render the direct light of every emitter of the scene, S shadow rays per pixel and round towards emitters picked by "
                         "power (default 1 round); with --probe-lit and --probe-gather: the final-gather split")
    ap.add_argument("--emitter-bias", type=float, default=None, metavar="B",
                    help="with --emitter-light: move shadow-ray origins B >= 0 world units along the normal (default 0.001)")
    opt = ap.parse_args(argv)
    emit = None
    if opt.emitter_light is not None:
        if opt.area_light is not None:
            ap.error("--emitter-light cannot be combined with --area-light: the area lights are among the emitters and would be sampled twice")
        if opt.probe_lit is not None and opt.probe_gather is None:
            ap.error("--probe-lit with --emitter-light needs --probe-gather: the probes already hold the emitters' direct light, so adding the "
                     "sampled emitters' to a probe lookup at the pixel would count it twice")
        if (opt.direct_light and opt.probe_lit is None) or opt.ao is not None or opt.bake_probes is not None or opt.bake_lightmap is not None \
                or opt.camera != "pinhole" or opt.denoise is not None or opt.orbit or opt.adaptive is not None or opt.progressive > 0 or opt.checkpoint \
                or opt.temporal is not None:
            ap.error("--emitter-light cannot be combined with --direct-light (without --probe-lit), --ao, --bake-probes, --bake-lightmap, --camera, "
                     "--denoise, --orbit, --adaptive, --progressive, --checkpoint or --temporal")
        try:
            emit = [int(x) for x in opt.emitter_light.split(",")]
        except ValueError:
            emit = []
        if not 1 <= len(emit) <= 2 or not 1 <= emit[0] <= 1 << 20 or (len(emit) == 2 and emit[1] < 1):
            ap.error("--emitter-light needs S[,ROUNDS]: 1 <= S <= 2^20, ROUNDS >= 1")
        if opt.emitter_bias is not None and not 0.0 <= opt.emitter_bias < float("inf"):
            ap.error("--emitter-bias B needs a finite B >= 0")
        if opt.aov_samples < 1:
            ap.error("--aov-samples needs S >= 1")
        if not opt.output:
            ap.error("--emitter-light needs -o FILE.png")
    elif opt.emitter_bias is not None:
        ap.error("--emitter-bias needs --emitter-light")
    area = None
    if opt.area_light is not None:
        if opt.probe_lit is not None and opt.probe_gather is None:
            ap.error("--probe-lit with --area-light needs --probe-gather: the probes already hold the emitters' direct light, so adding the "
                     "area lights' to a probe lookup at the pixel would count it twice")
        if (opt.direct_light and opt.probe_lit is None) or opt.ao is not None or opt.bake_probes is not None or opt.bake_lightmap is not None \
                or opt.camera != "pinhole" or opt.denoise is not None or opt.orbit or opt.adaptive is not None or opt.progressive > 0 or opt.checkpoint \
                or opt.temporal is not None:
            ap.error("--area-light cannot be combined with --direct-light (without --probe-lit), --ao, --bake-probes, --bake-lightmap, --camera, "
                     "--denoise, --orbit, --adaptive, --progressive, --checkpoint or --temporal")
        try:
            area = [int(x) for x in opt.area_light.split(",")]
        except ValueError:
            area = []
        if not 1 <= len(area) <= 2 or not 1 <= area[0] <= 1 << 20 or (len(area) == 2 and area[1] < 1):
            ap.error("--area-light needs S[,ROUNDS]: 1 <= S <= 2^20, ROUNDS >= 1")
        if opt.area_bias is not None and not 0.0 <= opt.area_bias < float("inf"):
            ap.error("--area-bias B needs a finite B >= 0")
        if opt.aov_samples < 1:
            ap.error("--aov-samples needs S >= 1")
        if not opt.output:
            ap.error("--area-light needs -o FILE.png")
    elif opt.area_bias is not None:
        ap.error("--area-bias needs --area-light")
    reflect = None
    if opt.probe_reflect is not None:
        if opt.probe_lit is None:
            ap.error("--probe-reflect needs --probe-lit")
        if opt.ao is not None:
            ap.error("--probe-reflect cannot be combined with --ao: the ambient-occlusion frame has no specular term")
        if opt.probe_split_sum is not None:
            ap.error("--probe-reflect cannot be combined with --probe-split-sum: the reflection rays' weights carry that term already")
        try:
            reflect = [int(x) for x in opt.probe_reflect.split(",")]
        except ValueError:
            reflect = []
        if not 1 <= len(reflect) <= 2 or not 1 <= reflect[0] <= 1 << 20 or (len(reflect) == 2 and reflect[1] < 1):
            ap.error("--probe-reflect needs D[,ROUNDS]: 1 <= D <= 2^20, ROUNDS >= 1")
        if opt.reflect_bias is not None and not 0.0 <= opt.reflect_bias < float("inf"):
            ap.error("--reflect-bias B needs a finite B >= 0")
    elif opt.reflect_bias is not None:
        ap.error("--reflect-bias needs --probe-reflect")
    gather = None
    if opt.probe_gather is not None:
        if opt.probe_lit is None:
            ap.error("--probe-gather needs --probe-lit")
        if opt.ao is not None:
            ap.error("--probe-gather cannot be combined with --ao: the gather rays find the occluders themselves")
        if opt.probe_split_sum is not None:
            ap.error("--probe-gather cannot be combined with --probe-split-sum: the gathered frame has no specular term")
        try:
            gather = [int(x) for x in opt.probe_gather.split(",")]
        except ValueError:
            gather = []
        if not 1 <= len(gather) <= 2 or not 1 <= gather[0] <= 1 << 20 or (len(gather) == 2 and gather[1] < 1):
            ap.error("--probe-gather needs D[,ROUNDS]: 1 <= D <= 2^20, ROUNDS >= 1")
        if opt.gather_bias is not None and not 0.0 <= opt.gather_bias < float("inf"):
            ap.error("--gather-bias B needs a finite B >= 0")
    elif opt.gather_bias is not None:
        ap.error("--gather-bias needs --probe-gather")
    split_sum = None
    if opt.probe_split_sum is not None:
        if opt.probe_lit is None:
            ap.error("--probe-split-sum needs --probe-lit")
        if opt.probe_no_radiance:
            ap.error("--probe-split-sum cannot be combined with --probe-no-radiance: the term multiplies the radiance maps' lookup")
        try:
            split_sum = [int(x) for x in opt.probe_split_sum.split(",")]
        except ValueError:
            split_sum = []
        if len(split_sum) != 2 or not all(2 <= x <= 256 for x in split_sum):
            ap.error("--probe-split-sum needs N_MU,N_RHO, each in 2..256")
    elif opt.probe_energy:
        ap.error("--probe-energy needs --probe-split-sum")
    sun_sky = None
    if opt.sun_sky is not None:
        try:
            sun_sky = [float(x) for x in opt.sun_sky.split(",")]
        except ValueError:
            sun_sky = []
        if not 2 <= len(sun_sky) <= 3 or not all(abs(x) < float("inf") for x in sun_sky) or not -90.0 <= sun_sky[0] <= 90.0:
            ap.error("--sun-sky needs EL,AZ[,TURBIDITY]: finite numbers, EL in [-90, 90] degrees")
        if len(sun_sky) == 3 and not 0.0 <= sun_sky[2] <= 64.0:
            ap.error("--sun-sky TURBIDITY needs 0 <= TURBIDITY <= 64")
        sun_sky_size = [2048, 1024]
        if opt.sun_sky_size is not None:
            try:
                sun_sky_size = [int(x) for x in opt.sun_sky_size.split(",")]
            except ValueError:
                sun_sky_size = []
            if len(sun_sky_size) != 2 or not all(2 <= x <= 32768 for x in sun_sky_size):
                ap.error("--sun-sky-size needs W,H, each in 2..32768")
        if opt.sun == "light" and opt.env_sampling:       # delta lights and environment sampling together are FW_ERR_UNSUPPORTED
            ap.error("--sun light cannot be combined with --env-sampling: pass --sun disc for the map's own sun to be sampled")
    elif opt.sun_sky_size is not None or opt.sun is not None:
        ap.error("--sun-sky-size and --sun need --sun-sky")
    if opt.direct_light:
        if (opt.ao is not None or opt.bake_probes is not None or opt.bake_lightmap is not None or opt.camera != "pinhole" or opt.denoise is not None
                or opt.orbit or opt.adaptive is not None or opt.progressive > 0 or opt.checkpoint or opt.temporal is not None):
            ap.error("--direct-light cannot be combined with --ao, --bake-probes, --bake-lightmap, --camera, --denoise, --orbit, --adaptive, "
                     "--progressive, --checkpoint or --temporal")
        if opt.aov_samples < 1:
            ap.error("--aov-samples needs S >= 1")
        if not opt.output:
            ap.error("--direct-light needs -o FILE.png")
    if opt.lightmap_direct and opt.bake_lightmap is None:
        ap.error("--lightmap-direct needs --bake-lightmap")
    if opt.direct_bias is not None:
        if not (opt.direct_light or opt.lightmap_direct):
            ap.error("--direct-bias needs --direct-light or --lightmap-direct")
        if not 0.0 <= opt.direct_bias < float("inf"):
            ap.error("--direct-bias B needs a finite B >= 0")
    if opt.ao is not None:
        if (opt.probe_lit is not None or opt.bake_probes is not None or opt.bake_lightmap is not None or opt.camera != "pinhole"
                or opt.denoise is not None or opt.orbit or opt.adaptive is not None or opt.progressive > 0 or opt.checkpoint or opt.temporal is not None):
            ap.error("--ao cannot be combined with --probe-lit, --bake-probes, --bake-lightmap, --camera, --denoise, --orbit, --adaptive, "
                     "--progressive, --checkpoint or --temporal")
        if not 0.0 < opt.ao < float("inf"):
            ap.error("--ao RADIUS needs a finite RADIUS > 0")
        if opt.ao_dirs is not None and not 1 <= opt.ao_dirs <= 1 << 20:
            ap.error("--ao-dirs D needs 1 <= D <= 2^20")
        if opt.ao_rounds is not None and opt.ao_rounds < 1:
            ap.error("--ao-rounds R needs R >= 1")
        if opt.aov_samples < 1:
            ap.error("--aov-samples needs S >= 1")
        if not opt.output:
            ap.error("--ao needs -o FILE.png")
    elif opt.ao_dirs is not None or opt.ao_rounds is not None:
        ap.error("--ao-dirs and --ao-rounds need --ao")
    elif opt.ao_falloff and opt.lightmap_ao is None:
        ap.error("--ao-falloff needs --ao or --lightmap-ao")
    if opt.lightmap_ao is not None:
        if opt.bake_lightmap is None:
            ap.error("--lightmap-ao needs --bake-lightmap")
        if not 0.0 < opt.lightmap_ao < float("inf"):
            ap.error("--lightmap-ao RADIUS needs a finite RADIUS > 0")
    if opt.probe_lit is not None:
        if (opt.bake_probes is not None or opt.bake_lightmap is not None or opt.camera != "pinhole" or opt.denoise is not None or opt.orbit
                or opt.adaptive is not None or opt.progressive > 0 or opt.checkpoint or opt.temporal is not None):
            ap.error("--probe-lit cannot be combined with --bake-probes, --bake-lightmap, --camera, --denoise, --orbit, --adaptive, "
                     "--progressive, --checkpoint or --temporal")
        if opt.aov_samples < 1:
            ap.error("--aov-samples needs S >= 1")
        if not opt.output:
            ap.error("--probe-lit needs -o FILE.png")
        if opt.probe_normal_bias is not None and not 0.0 <= opt.probe_normal_bias < float("inf"):
            ap.error("--probe-normal-bias B needs a finite B >= 0")
    elif opt.probe_no_wrap:
        ap.error("--probe-no-wrap needs --probe-lit")
    elif opt.probe_no_placement:
        ap.error("--probe-no-placement needs --probe-lit")
    elif opt.probe_no_visibility or opt.probe_normal_bias is not None:
        ap.error("--probe-no-visibility and --probe-normal-bias need --probe-lit")
    if opt.bake_lightmap is not None:
        if (opt.bake_probes is not None or opt.camera != "pinhole" or opt.denoise is not None or opt.orbit or opt.adaptive is not None
                or opt.progressive > 0 or opt.checkpoint or opt.temporal is not None):
            ap.error("--bake-lightmap cannot be combined with --bake-probes, --camera, --denoise, --orbit, --adaptive, --progressive, "
                     "--checkpoint or --temporal")
        try:
            lm_args = [int(x) for x in opt.bake_lightmap.split(",")]
        except ValueError:
            lm_args = []
        if len(lm_args) != 3 or lm_args[0] < 0 or not all(1 <= x <= 16384 for x in lm_args[1:]):
            ap.error("--bake-lightmap needs OBJECT,W,H: an object index >= 0 and a size of 1..16384 each way")
        if opt.lightmap_dirs is not None and not 1 <= opt.lightmap_dirs <= 1 << 20:
            ap.error("--lightmap-dirs D needs 1 <= D <= 2^20")
        if opt.lightmap_rounds is not None and opt.lightmap_rounds < 1:
            ap.error("--lightmap-rounds R needs R >= 1")
        if opt.lightmap_dilate is not None and not 0 <= opt.lightmap_dilate <= 64:
            ap.error("--lightmap-dilate N needs 0 <= N <= 64")
        if not opt.output:
            ap.error("--bake-lightmap needs -o FILE.npz")
    elif opt.lightmap_dirs is not None or opt.lightmap_rounds is not None or opt.lightmap_dilate is not None:
        ap.error("--lightmap-dirs, --lightmap-rounds and --lightmap-dilate need --bake-lightmap")
    if opt.bake_probes is not None:
        if (opt.camera != "pinhole" or opt.denoise is not None or opt.orbit or opt.adaptive is not None or opt.progressive > 0 or opt.checkpoint
                or opt.temporal is not None):
            ap.error("--bake-probes cannot be combined with --camera, --denoise, --orbit, --adaptive, --progressive, --checkpoint or --temporal")
        try:
            counts = [int(x) for x in opt.bake_probes.split(",")]
        except ValueError:
            counts = []
        if len(counts) != 3 or min(counts) < 1:
            ap.error("--bake-probes needs NX,NY,NZ, three counts >= 1")
        corners = []
        for name, text in (("--probe-min", opt.probe_min), ("--probe-max", opt.probe_max)):
            try:
                c = [float(x) for x in (text or "").split(",")]
            except ValueError:
                c = []
            if len(c) != 3 or not all(abs(x) < float("inf") for x in c):
                ap.error(f"--bake-probes needs {name} x,y,z, three finite numbers")
            corners.append(c)
        if opt.probe_dirs is not None and not 1 <= opt.probe_dirs <= 1 << 20:
            ap.error("--probe-dirs D needs 1 <= D <= 2^20")
        if opt.probe_rounds is not None and opt.probe_rounds < 1:
            ap.error("--probe-rounds R needs R >= 1")
        if opt.probe_depth is not None:
            if opt.probe_depth not in (4, 8, 16, 32):
                ap.error("--probe-depth R needs R in 4, 8, 16, 32")
            if opt.probe_depth_sharpness is not None and not 0 <= opt.probe_depth_sharpness <= 8:
                ap.error("--probe-depth-sharpness K needs 0 <= K <= 8")
            if opt.probe_depth_max is not None and not 0.0 < opt.probe_depth_max < float("inf"):
                ap.error("--probe-depth-max M needs a finite M > 0")
            if opt.probe_depth_max is None and corners[0] == corners[1]:
                ap.error("--probe-depth needs --probe-depth-max M for a grid of one point: it has no diagonal")
        elif opt.probe_depth_sharpness is not None or opt.probe_depth_max is not None:
            ap.error("--probe-depth-sharpness and --probe-depth-max need --probe-depth")
        radiance_roughness = None
        if opt.probe_radiance is not None:
            if opt.probe_radiance not in (4, 8, 16, 32):
                ap.error("--probe-radiance R needs R in 4, 8, 16, 32")
            if opt.probe_radiance_sharpness is not None and not 0 <= opt.probe_radiance_sharpness <= 8:
                ap.error("--probe-radiance-sharpness K needs 0 <= K <= 8")
            if opt.probe_radiance_roughness is not None:
                try:
                    radiance_roughness = [float(x) for x in opt.probe_radiance_roughness.split(",")]
                except ValueError:
                    radiance_roughness = []
                most = min(4, opt.probe_radiance.bit_length() - 2)
                if (not 1 <= len(radiance_roughness) <= most or not all(0.0 <= x <= 1.0 for x in radiance_roughness)
                        or any(b <= a for a, b in zip(radiance_roughness, radiance_roughness[1:]))):
                    ap.error(f"--probe-radiance-roughness needs 1 to {most} numbers in [0, 1], strictly ascending")
        elif opt.probe_radiance_sharpness is not None or opt.probe_radiance_roughness is not None:
            ap.error("--probe-radiance-sharpness and --probe-radiance-roughness need --probe-radiance")
        if opt.probe_relocate is not None:
            if not 0.0 < opt.probe_relocate < float("inf"):
                ap.error("--probe-relocate MIN_FRONT needs a finite MIN_FRONT > 0")
            if opt.probe_relocate_steps is not None and not 0 <= opt.probe_relocate_steps < 1 << 31:
                ap.error("--probe-relocate-steps K needs K >= 0")
            if opt.probe_relocate_max is not None and not 0.0 <= opt.probe_relocate_max < float("inf"):
                ap.error("--probe-relocate-max F needs a finite F >= 0")
            if max(counts) == 1:
                ap.error("--probe-relocate needs a grid of more than one probe: a single point has no spacing")
        elif opt.probe_relocate_steps is not None or opt.probe_relocate_max is not None:
            ap.error("--probe-relocate-steps and --probe-relocate-max need --probe-relocate")
        if not opt.output:
            ap.error("--bake-probes needs -o FILE.npz")
    elif opt.probe_min is not None or opt.probe_max is not None or opt.probe_dirs is not None or opt.probe_rounds is not None:
        ap.error("--probe-min, --probe-max, --probe-dirs and --probe-rounds need --bake-probes")
    elif opt.probe_depth is not None or opt.probe_depth_sharpness is not None or opt.probe_depth_max is not None:
        ap.error("--probe-depth, --probe-depth-sharpness and --probe-depth-max need --bake-probes")
    elif opt.probe_relocate is not None or opt.probe_relocate_steps is not None or opt.probe_relocate_max is not None:
        ap.error("--probe-relocate, --probe-relocate-steps and --probe-relocate-max need --bake-probes")
    elif opt.probe_radiance is not None or opt.probe_radiance_sharpness is not None or opt.probe_radiance_roughness is not None:
        ap.error("--probe-radiance, --probe-radiance-sharpness and --probe-radiance-roughness need --bake-probes")
    if opt.adaptive is not None and (opt.progressive > 0 or opt.checkpoint):
        ap.error("--adaptive cannot be combined with --progressive or --checkpoint")
    if opt.temporal is not None:
        if opt.progressive > 0 or opt.checkpoint or opt.adaptive is not None or opt.camera != "pinhole":
            ap.error("--temporal cannot be combined with --progressive, --checkpoint, --adaptive or --camera")
        if opt.orbit <= 0:
            ap.error("--temporal needs --orbit N: it merges each view with the one before it")
        if not opt.temporal > 0:
            ap.error("--temporal MAX_HISTORY needs MAX_HISTORY > 0")
    if opt.denoise is not None:
        if opt.progressive > 0 or opt.checkpoint or (opt.orbit and opt.temporal is None):
            ap.error("--denoise cannot be combined with --progressive, --checkpoint or --orbit")
        if not 0 <= opt.denoise <= 10:
            ap.error("--denoise L needs 0 <= L <= 10")
        if opt.aov_samples < 1:
            ap.error("--aov-samples needs S >= 1")
    if opt.orbit < 0:
        ap.error("--orbit N needs N >= 1")
    if opt.camera != "pinhole":
        if opt.orbit or opt.adaptive is not None or opt.denoise is not None or opt.progressive > 0 or opt.checkpoint:
            ap.error(f"--camera {opt.camera} cannot be combined with --orbit, --adaptive, --denoise, --progressive or --checkpoint")
        if opt.ortho_height is not None and not opt.ortho_height > 0:
            ap.error("--ortho-height H needs H > 0")
    elif opt.ortho_height is not None:
        ap.error("--ortho-height needs --camera orthographic")
    if opt.fisheye_fov is not None:
        if opt.camera != "fisheye":
            ap.error("--fisheye-fov needs --camera fisheye")
        if not 0.0 < opt.fisheye_fov <= 360.0:
            ap.error("--fisheye-fov DEG needs 0 < DEG <= 360")
    if opt.orbit > 0:
        if opt.progressive > 0 or opt.checkpoint or opt.adaptive is not None:
            ap.error("--orbit cannot be combined with --progressive, --checkpoint or --adaptive")
        try:
            names = view_paths(opt.output, opt.orbit)
        except (TypeError, ValueError, IndexError, KeyError):
            names = None
        if names is None:
            ap.error("--orbit needs -o with a format field for the view number, e.g. -o 'frame_{:03d}.png'")

    from . import _lib
    from .api import CameraSettings, Renderer, save_image
    from .yaml_io import load_scene

    scene = lightmap = None
    if opt.bake_lightmap is not None:      # the object is looked at before the device is: a wrong one is a message, not a traceback
        from .api import Lightmap
        scene = load_scene(opt.scene_file)
        try:
            lightmap = Lightmap.of(scene, lm_args[0], lm_args[1], lm_args[2], 64 if opt.lightmap_dirs is None else opt.lightmap_dirs).seed(opt.seed)
        except ValueError as e:
            print(f"firework: error: --bake-lightmap: {e}", file=sys.stderr)
            return 2

    probe_grid = probe_sh = probe_depth = probe_moments = probe_placement = probe_radiance = probe_maps = None
    if opt.probe_lit is not None:          # the file is looked at before the device is: a wrong one is a message, not a traceback
        import zipfile
        import numpy as np
        from .api import ProbeGrid
        try:
            with np.load(opt.probe_lit) as z:
                missing = [k for k in ("sh", "grid_lo", "grid_hi", "grid_counts") if k not in z.files]
                if missing:
                    raise ValueError(f"no {', '.join(missing)} in it (bake it with this version's --bake-probes: only a grid can be looked up)")
                probe_grid = ProbeGrid(z["grid_lo"], z["grid_hi"], z["grid_counts"], not opt.probe_no_wrap)
                probe_sh = np.asarray(z["sh"], np.float32)
                if "depth" in z.files and not opt.probe_no_visibility:
                    from .api import ProbeDepth
                    missing = [k for k in ("depth_res", "depth_sharpness", "depth_max") if k not in z.files]
                    if missing:
                        raise ValueError(f"depth without {', '.join(missing)} in it")
                    probe_depth = ProbeDepth(int(z["depth_res"]), int(z["depth_sharpness"]), float(z["depth_max"]))
                    probe_moments = np.asarray(z["depth"], np.float32)
                if "placement" in z.files and not opt.probe_no_placement:
                    probe_placement = np.asarray(z["placement"], np.float32)
                if "radiance" in z.files and not opt.probe_no_radiance:
                    from .api import ProbeRadiance
                    missing = [k for k in ("radiance_res", "radiance_sharpness", "radiance_roughness") if k not in z.files]
                    if missing:
                        raise ValueError(f"radiance without {', '.join(missing)} in it")
                    probe_radiance = ProbeRadiance(int(z["radiance_res"]), int(z["radiance_sharpness"]), np.asarray(z["radiance_roughness"], np.float32))
                    probe_maps = np.asarray(z["radiance"], np.float32)
            if probe_sh.shape != (probe_grid.n_probes, 9, 3):
                raise ValueError(f"sh has shape {probe_sh.shape}, the grid {probe_grid.n_probes} probes")
            if probe_depth is not None and probe_moments.shape != (probe_grid.n_probes, probe_depth.resolution, probe_depth.resolution, 2):
                raise ValueError(f"depth has shape {probe_moments.shape}, the grid {probe_grid.n_probes} probes of resolution {probe_depth.resolution}")
            if probe_placement is not None and probe_placement.shape != (probe_grid.n_probes, 4):
                raise ValueError(f"placement has shape {probe_placement.shape}, the grid {probe_grid.n_probes} probes")
            if probe_radiance is not None and probe_maps.shape != (probe_grid.n_probes, probe_radiance.texels, 4):
                raise ValueError(f"radiance has shape {probe_maps.shape}, the grid {probe_grid.n_probes} probes of {probe_radiance.texels} texels")
            if gather is not None and probe_radiance is not None:
                raise ValueError("--probe-gather cannot be combined with the radiance maps the file holds: pass --probe-no-radiance")
            if reflect is not None and probe_radiance is not None:
                raise ValueError("--probe-reflect cannot be combined with the radiance maps the file holds: pass --probe-no-radiance")
            if split_sum is not None and probe_radiance is None:
                raise ValueError("--probe-split-sum needs radiance maps and the file holds none (bake it with --probe-radiance R)")
        except (OSError, ValueError, zipfile.BadZipFile) as e:
            print(f"firework: error: --probe-lit {opt.probe_lit}: {e}", file=sys.stderr)
            return 2

    _lib.init(opt.device)      # fw_init: context, code objects and the path arena before the timed region, like the loading of the reference's binary (main.rs:40)

    if scene is None:
        scene = load_scene(opt.scene_file)
    if sun_sky is not None:
        from .api import SunSky, SunSkyEnv
        scene.set_environment(SunSkyEnv(SunSky(sun_sky[0], sun_sky[1], *sun_sky[2:]), sun_sky_size[0], sun_sky_size[1], opt.sun or "disc"))
    camera =CameraSettings.default().cam_pos((0.0, 30.0, 50.0)).look_at((0.0, 0.0, 0.0)).field_of_view(40.0)
    renderer = (Renderer.default().width(opt.width).height(opt.height).samples(opt.samples).use_bvh(True)
                .camera(camera).seed(opt.seed).light_sampling(opt.light_sampling).env_sampling(opt.env_sampling))
    if opt.all_emitters:       # bits 4 and 16: light sampling over every emitting primitive
        renderer.light_sampling().all_emitters()
    start = time.time()
    if opt.bake_probes is not None:
        import numpy as np
        from .api import ProbeSet
        probes = ProbeSet.grid(corners[0], corners[1], counts, 256 if opt.probe_dirs is None else opt.probe_dirs).seed(opt.seed)
        rounds = 1 if opt.probe_rounds is None else opt.probe_rounds
        extra = {}
        nominal = probes
        if opt.probe_relocate is not None:      # first: sh and depth are then baked where the probes went
            from .api import ProbeRelocation, probe_spacing
            fraction = 0.45 if opt.probe_relocate_max is None else opt.probe_relocate_max
            relocation = ProbeRelocation(opt.probe_relocate, max_offset=tuple(fraction * v for v in probe_spacing(probes)),
                                         steps=4 if opt.probe_relocate_steps is None else opt.probe_relocate_steps)
            placement, _survey = renderer.relocate_probes(scene, probes, relocation, device=opt.device)
            print(f"Relocated {int(np.any(placement[:, 0:3] != 0, axis=1).sum())} probes, {int((placement[:, 3] == 0).sum())} inactive")
            extra = dict(placement=placement, relocate_min_front=np.float32(relocation.min_front), relocate_steps=np.int64(relocation.steps))
            probes = nominal.moved(placement)
        if opt.probe_radiance is not None:      # one render pass for the SH and the maps: the same sh and sums, bit for bit
            from .api import ProbeRadiance
            radiance = ProbeRadiance(opt.probe_radiance, 2 if opt.probe_radiance_sharpness is None else opt.probe_radiance_sharpness, radiance_roughness)
            maps, _radiance_sums, sh, sums = renderer.bake_probe_radiance(scene, probes, radiance, rounds, chunk=None, with_sh=True, device=opt.device)
            extra.update(radiance=maps, radiance_res=np.int64(radiance.resolution), radiance_sharpness=np.int64(radiance.sharpness_log2),
                         radiance_roughness=np.array(radiance.roughness, np.float32))
        else:
            sh, sums = renderer.bake_probes(scene, probes, rounds, device=opt.device)
        if opt.probe_depth is not None:
            from .api import ProbeDepth
            diagonal = float(np.sqrt(sum((b - a) ** 2 for a, b in zip(corners[0], corners[1]))))
            depth = ProbeDepth(opt.probe_depth, 6 if opt.probe_depth_sharpness is None else opt.probe_depth_sharpness,
                               diagonal if opt.probe_depth_max is None else opt.probe_depth_max)
            moments, _depth_sums = renderer.bake_probe_depth(scene, probes, depth, rounds, device=opt.device)
            extra.update(depth=moments, depth_res=np.int64(depth.resolution), depth_sharpness=np.int64(depth.sharpness_log2),
                          depth_max=np.float32(depth.max_distance))
        print(f"Finished Baking in {int(time.time() - start)} s")
        print(f'Saving {probes.n_probes} probes to "{opt.output}"')
        with open(opt.output, "wb") as f:       # (np.savez would append .npz to a name without it)
            np.savez(f, positions=nominal.positions, sh=sh, sums=sums, rounds=np.int64(rounds), directions=np.int64(probes.directions),
                     samples=np.int64(opt.samples), grid_lo=np.array(probes.grid_lo, np.float64), grid_hi=np.array(probes.grid_hi, np.float64),
                     grid_counts=np.array(probes.grid_counts, np.int64), **extra)
        return 0
    if probe_grid is not None:
        ggx_table = None
        if split_sum is not None:
            from .api import GgxTable
            ggx_table = GgxTable(split_sum[0], split_sum[1], energy=opt.probe_energy)
        final_gather = None
        if gather is not None:
            from .api import FinalGather
            final_gather = FinalGather(gather[0], 1e-3 if opt.gather_bias is None else opt.gather_bias).seed(opt.seed)
        area_light = None
        if area is not None:
            from .api import AreaLight
            area_light = AreaLight(area[0], 1e-3 if opt.area_bias is None else opt.area_bias).seed(opt.seed)
        emitter_lights = None
        if emit is not None:
            from .api import EmitterLights
            emitter_lights = EmitterLights(emit[0], 1e-3 if opt.emitter_bias is None else opt.emitter_bias).seed(opt.seed)
        reflection = None
        if reflect is not None:
            from .api import ReflectionGather
            reflection = ReflectionGather(reflect[0]).bias(1e-3 if opt.reflect_bias is None else opt.reflect_bias).seed(opt.seed)
        render = renderer.render_probe_lit(scene, probe_grid, probe_sh, opt.aov_samples, device=opt.device, depth=probe_depth, moments=probe_moments,
                                           normal_bias=0.0 if opt.probe_normal_bias is None else opt.probe_normal_bias,
                                           placement=probe_placement, radiance=probe_radiance, maps=probe_maps, direct=direct_light(opt),
                                           ggx_table=ggx_table, gather=final_gather, gather_rounds=gather[1] if gather and len(gather) == 2 else 1,
                                           reflect=reflection, reflect_rounds=reflect[1] if reflect and len(reflect) == 2 else 1,
                                           area=area_light, area_rounds=area[1] if area and len(area) == 2 else 1,
                                           emitters=emitter_lights, emitters_rounds=emit[1] if emit and len(emit) == 2 else 1).rgb8
        print(f"Finished Rendering in {int(time.time() - start)} s")
        print(f'Saving image to "{opt.output}"')
        save_image(render, opt.output, opt.width, opt.height)
        return 0
    if area is not None:
        from .api import AreaLight
        area_light = AreaLight(area[0], 1e-3 if opt.area_bias is None else opt.area_bias).seed(opt.seed)
        render = renderer.render_area(scene, area_light, area[1] if len(area) == 2 else 1, opt.aov_samples, device=opt.device).rgb8
        print(f"Finished Rendering in {int(time.time() - start)} s")
        print(f'Saving image to "{opt.output}"')
        save_image(render, opt.output, opt.width, opt.height)
        return 0
    if emit is not None:
        from .api import EmitterLights
        emitter_lights = EmitterLights(emit[0], 1e-3 if opt.emitter_bias is None else opt.emitter_bias).seed(opt.seed)
        render = renderer.render_emitters(scene, emitter_lights, emit[1] if len(emit) == 2 else 1, opt.aov_samples, device=opt.device).rgb8
        print(f"Finished Rendering in {int(time.time() - start)} s")
        print(f'Saving image to "{opt.output}"')
        save_image(render, opt.output, opt.width, opt.height)
        return 0
    if opt.direct_light:
        render = renderer.render_direct(scene, direct_light(opt), opt.aov_samples, device=opt.device).rgb8
        print(f"Finished Rendering in {int(time.time() - start)} s")
        print(f'Saving image to "{opt.output}"')
        save_image(render, opt.output, opt.width, opt.height)
        return 0
    if opt.ao is not None:
        import numpy as np
        from .api import AmbientOcclusion
        ao = AmbientOcclusion(opt.ao, 64 if opt.ao_dirs is None else opt.ao_dirs, int(opt.ao_falloff)).seed(opt.seed)
        occ, _bent, _sums = renderer.render_ao(scene, ao, 1 if opt.ao_rounds is None else opt.ao_rounds, opt.aov_samples, device=opt.device)
        grey = np.clip(np.floor(occ * np.float32(255.99)), 0, 255).astype(np.uint8)
        print(f"Finished Rendering in {int(time.time() - start)} s")
        print(f'Saving image to "{opt.output}"')
        save_image(np.repeat(grey.reshape(-1, 1), 3, axis=1), opt.output, opt.width, opt.height)
        return 0
    if lightmap is not None:
        import numpy as np
        rounds = 1 if opt.lightmap_rounds is None else opt.lightmap_rounds
        irradiance, sums = renderer.bake_lightmap(scene, lightmap, rounds, 2 if opt.lightmap_dilate is None else opt.lightmap_dilate, device=opt.device,
                                                  direct=direct_light(opt, opt.lightmap_direct))
        owner = _lib.lightmap_texels(lightmap, opt.device)[1].reshape(lightmap.height, lightmap.width)
        extra = {}
        if opt.lightmap_direct:
            extra = dict(direct=renderer.lightmap_direct)
        if opt.lightmap_ao is not None:
            from .api import AmbientOcclusion
            ao = AmbientOcclusion(opt.lightmap_ao, lightmap.directions, int(opt.ao_falloff)).seed(opt.seed)
            occ, bent, _ao_sums = renderer.bake_lightmap_ao(scene, lightmap, ao, rounds, 2 if opt.lightmap_dilate is None else opt.lightmap_dilate,
                                                            device=opt.device)
            extra.update(ao=occ, bent=bent)
        print(f"Finished Baking in {int(time.time() - start)} s")
        print(f'Saving a {lightmap.width} x {lightmap.height} lightmap to "{opt.output}"')
        with open(opt.output, "wb") as f:       # (np.savez would append .npz to a name without it)
            np.savez(f, irradiance=irradiance, sums=sums, owner=owner, rounds=np.int64(rounds), directions=np.int64(lightmap.directions),
                     samples=np.int64(opt.samples), **extra)
        return 0
    if opt.camera != "pinhole":
        render = camera_model_render(renderer, camera, scene, opt)
    elif opt.orbit > 0 and opt.temporal is not None:
        from .api import orbit_cameras
        frames = renderer.render_sequence(scene, orbit_cameras(camera, opt.orbit), device=opt.device, max_history=opt.temporal,
                                          iterations=5 if opt.denoise is None else opt.denoise, aov_samples=opt.aov_samples)
        for name, res in zip(names, frames):
            save_image(res.rgb8, name, opt.width, opt.height)
        print(f"Finished Rendering in {int(time.time() - start)} s")
        print(f'Saved {opt.orbit} views to "{names[0]}" .. "{names[-1]}"')
        return 0
    elif opt.orbit > 0:
        from .api import orbit_cameras
        res = renderer.render_views(scene, orbit_cameras(camera, opt.orbit), device=opt.device)
        print(f"Finished Rendering in {int(time.time() - start)} s")
        for name, img in zip(names, res.rgb8):
            save_image(img, name, opt.width, opt.height)
        print(f'Saved {opt.orbit} views to "{names[0]}" .. "{names[-1]}"')
        return 0
    if opt.camera != "pinhole":
        pass
    elif opt.denoise is not None:
        render = denoised(renderer, scene, opt)
    elif opt.adaptive is not None:
        res = renderer.render_adaptive(scene, opt.adaptive, opt.min_samples, device=opt.device)
        render = res.rgb8
        print(f"adaptive: {len(res.rounds)} rounds, active pixels {res.rounds}, mean {float(res.counts.mean()):.1f} spp (cap {opt.samples})")
    elif opt.progressive > 0 or opt.checkpoint:
        render = None
        for k, res in enumerate(renderer.render_progressive(scene, max(1, opt.progressive), device=opt.device, checkpoint=opt.checkpoint)):
            render = res.rgb8
            if opt.output:
                save_image(render, opt.output, opt.width, opt.height)
            print(f"pass {k + 1}: {int(time.time() - start)} s")
        if render is None:          # the checkpoint already held every sample
            render = renderer.render(scene, device=opt.device)
    else:
        render = renderer.render(scene, device=opt.device)
    print(f"Finished Rendering in {int(time.time() - start)} s")
    if opt.output:
        print(f'Saving image to "{opt.output}"')
        save_image(render, opt.output, opt.width, opt.height)
    else:
        name = opt.name or "Firework Render"
        print(f"{name}: no display on this node; pass -o/--output to save the image", file=sys.stderr)
        return 2
    return 0


def direct_light(opt, on=None):
    """the DirectLight of --direct-light (or of `on`), or None"""
    if not (opt.direct_light if on is None else on):
        return None
    from .api import DirectLight
    return DirectLight(1e-3 if opt.direct_bias is None else opt.direct_bias)


def denoised(renderer, scene, opt):
    """--denoise: the frame (a plain render, or --adaptive's with its moments and per-pixel counts) filtered by fw_denoise; returns rgb8."""
    from . import _lib
    if opt.adaptive is None:
        return renderer.render_denoised(scene, opt.denoise, opt.aov_samples, device=opt.device).rgb8
    ds = _lib.DeviceScene(scene.to_desc(), opt.device)
    try:
        res = ds.render_adaptive(renderer, opt.adaptive, opt.min_samples)
        print(f"adaptive: {len(res.rounds)} rounds, active pixels {res.rounds}, mean {float(res.counts.mean()):.1f} spp (cap {opt.samples})")
        aov = ds.aovs(renderer, opt.aov_samples)
    finally:
        ds.close()
    return _lib.denoise(res.linear, aov, res.moments, opt.width, opt.height, opt.denoise, renderer.settings["gamma"], opt.device)[0]


def camera_model_render(renderer, camera, scene, opt):
    """--camera panorama / orthographic / fisheye: the model's rays are generated on the device, chunk by chunk of samples, and rendered
    by fw_render_model; returns rgb8."""
    import math
    from .api import CameraModel
    if opt.camera == "panorama":
        model = CameraModel.panorama(camera._cam_pos, opt.width, opt.height)
    elif opt.camera == "fisheye":
        model = CameraModel.fisheye(camera, 180.0 if opt.fisheye_fov is None else opt.fisheye_fov, opt.width, opt.height)
    else:
        h = opt.ortho_height
        if h is None:       # the height the pinhole view sees at its look-at point
            dist = float(math.dist(camera._cam_pos.tolist(), camera._look_at.tolist()))
            h = 2.0 * math.tan(math.radians(camera._vfov) / 2.0) * dist
        model = CameraModel.orthographic(camera, h, opt.width, opt.height)
    return renderer.render_model(scene, model.seed(opt.seed), opt.samples, device=opt.device).image(opt.width, opt.height)


def view_paths(pattern, n):
    """--orbit's file names: `pattern` formatted with each view number 0..n-1; None unless the names differ between views."""
    if not pattern:
        return None
    names = [pattern.format(k) for k in range(max(n, 2))]
    return names[:n] if len(set(names)) == len(names) else None


if __name__ == "__main__":
    sys.exit(main())
