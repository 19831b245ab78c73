// render_gpu.go — the Go side of the drop-in boundary: Render on the MI355X path, a cgo binding of
// librtx.so (include/rtx.h) for TwFlem/raytracer-go.
//
// A maintainer copies this file into the reference's package `internal` (next to
// internal/camera.go; the Hittable/Material/Texture fields it flattens are unexported, so it
// must live in that package), adds the three-line hook at the top of Render (INTEGRATION.md:
// `if done, err := c.renderGPU(world, writer); done { return err }`) and points cgo at a build of
// this repository (`make -C raytracer-go_amd`) through the environment, wherever it is checked out:
//   CGO_CFLAGS="-I$RTX/include" CGO_LDFLAGS="-L$RTX/raytracer-go_amd -Wl,-rpath,$RTX/raytracer-go_amd" go build
// ($RTX = this repository's root).  main.go then changes only its camera options:
//   internal.NewCamera(16.0/9.0, 1920, ..., internal.WithGPUs(1), internal.WithSeed(2024))
// (or RTX_GPUS=1 in the environment, with no change at all), and, to build the BVH of a World of
// spheres and quads on the GPU instead of NewBVHFromWorld's host recursion (bvh.go:138-185; 100k spheres),
// internal.NewBVHFromWorldGPU(world) in place of internal.NewBVHFromWorld(world).
// Render keeps its CPU path for every scene part, device or option the GPU path does not carry.
//
// Go is not installed in the image this repository is built in, so this file has not been
// compiled; tests/test_go_binding.py checks every C identifier and struct field it names against
// include/rtx.h and drives the exact C-ABI call sequences it issues through ctypes, and the same
// flattening is built and tested in C++ (raytracer-go_amd/host/flatten.cpp).
package internal

/*
#cgo LDFLAGS: -lrtx
#include <stdlib.h>
#include "rtx.h"
*/
import "C"

import (
	"errors"
	"fmt"
	"io"
	"math"
	"os"
	"runtime"
	"strconv"
	"sync"
	"sync/atomic"
	"unsafe"
)

// gpuConfig holds a Camera's GPU options (WithGPUs, WithSeed).  The Camera struct is camera.go's,
// so they are kept beside it, keyed by the *Camera (a Camera lives as long as its program).
type gpuConfig struct {
	gpus     int
	seed     uint64
	noiseTol float32     // WithNoiseTolerance: RenderProgressive stops once no pixel is noisier (0: off)
	fallback atomic.Bool // RenderGPU is running the CPU Render: the hook stays out of the way
}

var gpuConfigs sync.Map // *Camera -> *gpuConfig

func (c *Camera) gpuConfig() *gpuConfig {
	if v, ok := gpuConfigs.Load(c); ok {
		return v.(*gpuConfig)
	}
	cfg := &gpuConfig{seed: 1}
	if n, err := strconv.Atoi(os.Getenv("RTX_GPUS")); err == nil { // the default without WithGPUs
		cfg.gpus = n
	}
	v, _ := gpuConfigs.LoadOrStore(c, cfg)
	return v.(*gpuConfig)
}

// WithGPUs renders on n MI355X devices of this process: Render runs the megakernel on row-
// interleaved bands of the image, one per device, gathered to device 0 over RCCL (n > 1).  0 keeps
// the reference's CPU path.  Without this option the RTX_GPUS environment variable decides.
func WithGPUs(n int) CameraOpt {
	return func(c *Camera) {
		c.gpuConfig().gpus = n
	}
}

// WithSeed keys the GPU path's counter-based RNG (Philox4x32-10; DESIGN.md §3): the same seed
// gives the same image on any number of devices.  (The CPU path seeds its workers from the clock,
// camera.go:170.)  It also seeds NewBVHFromWorldGPU's axis draws.
func WithSeed(seed uint64) CameraOpt {
	return func(c *Camera) {
		c.gpuConfig().seed = seed
	}
}

// WithNoiseTolerance makes RenderProgressive stop as soon as no pixel is noisy at the relative
// tolerance rel (rtx_accum_resolve: the summed variance of the pixel mean against (rel * max(r + g + b,
// 0.01))^2), before samplesPerPixel is reached.  0, the default, renders every sample.
func WithNoiseTolerance(rel float32) CameraOpt {
	return func(c *Camera) {
		c.gpuConfig().noiseTol = rel
	}
}

// gpuBVH is the tree NewBVHFromWorld would build over a World of spheres and quads, built on the
// GPU by rtx_scene_create_spheres, or by rtx_scene_create_world when the World holds a quad
// (NewBVH restated, bvh.go:142-185: the same sort and median split per
// node, the axis drawn from the render seed's stream instead of the global rand).  The CPU path
// (Hit, GetBounds) builds the reference's tree on first use.
type gpuBVH struct {
	world *World
	once  sync.Once
	tree  *BVH
}

// NewBVHFromWorldGPU stands in for NewBVHFromWorld (bvh.go:138-140) when the World holds only
// spheres and quads (Box's included): Render on the GPU path builds the tree on the device (10 ms for
// 100k spheres, where the host recursion takes about 0.5 s), and any CPU use builds the reference's
// tree.  A World holding anything else (a nested World, a BVH) renders on the CPU path.
func NewBVHFromWorldGPU(w *World) Hittable { return &gpuBVH{world: w} }

func (g *gpuBVH) cpu() *BVH {
	g.once.Do(func() { g.tree = NewBVHFromWorld(g.world) })
	return g.tree
}

func (g *gpuBVH) Hit(r *Ray, rayT Interval) (HitInfo, bool) { return g.cpu().Hit(r, rayT) }

func (g *gpuBVH) GetBounds() Aabb { return g.cpu().GetBounds() }

// gpuTables is the flattened Hittable tree (rtx.h).  The slices hold no Go pointers, so
// passing them to C is legal under the cgo rules; librtx copies them and never keeps them.
type gpuTables struct {
	nodes     []C.rtx_bvh_node
	roots     []C.int32_t
	spheres   []C.rtx_sphere
	quads     []C.rtx_quad
	materials []C.rtx_material
	textures  []C.rtx_texture
	texels    []C.uint32_t
	lists     []C.rtx_list  // Worlds nested in the tree (ABI 5)
	listRefs  []C.int32_t
	matIdx    map[Material]C.uint32_t
	texIdx    map[Texture]C.uint32_t
	// the Go values behind the table indices, for HitBatch: rtx_hit.prim and .material back to what was flattened
	sphereOf   []*Sphere
	quadOf     []Quad
	materialOf []Material
}

// errUnsupported: a scene part the GPU path does not carry (RenderGPU then uses Render).
var errUnsupported = errors.New("rtx: scene type not on the GPU path")

func primRef(typ, idx int) C.int32_t { return C.int32_t(^int32(uint32(typ)<<28 | uint32(idx)&0x0FFFFFFF)) }

func vec(v Vec3) [3]C.float { return [3]C.float{C.float(v.X), C.float(v.Y), C.float(v.Z)} }

// putRGBA16 appends one RTX_TEX_IMAGE texel: Go's 16-bit Color.RGBA() channels, two words.
func (t *gpuTables) putRGBA16(r, g, b, a uint32) {
	t.texels = append(t.texels, C.uint32_t(r&0xFFFF|(g&0xFFFF)<<16), C.uint32_t(b&0xFFFF|(a&0xFFFF)<<16))
}

func (t *gpuTables) texture(tex Texture) (C.uint32_t, error) {
	if i, ok := t.texIdx[tex]; ok {
		return i, nil
	}
	var r C.rtx_texture
	switch v := tex.(type) {
	case SolidColor:
		r._type, r.even = C.RTX_TEX_SOLID, vec(v.albedo.GetColor())
	case *SolidColor:
		r._type, r.even = C.RTX_TEX_SOLID, vec(v.albedo.GetColor())
	case *Checkered:
		r._type, r.scale = C.RTX_TEX_CHECKERED, C.float(v.scale)
		r.even, r.odd = vec(v.even.GetColor()), vec(v.odd.GetColor())
	case *ImageTexture: // materials.go:175-193: At(int(u*Dx), int(v*Dy)).RGBA(), 16 bits per channel
		b := v.img.Bounds()
		r._type = C.RTX_TEX_IMAGE
		if b.Dy() > 0 {
			// GetTexture indexes At from 0; the table (and its border texel) is exact for bounds
			// at the origin, which jpeg.Decode and image.New* return.
			if b.Min.X != 0 || b.Min.Y != 0 {
				return 0, errUnsupported
			}
			r.width, r.height = C.uint32_t(b.Dx()), C.uint32_t(b.Dy())
			if len(t.texels)%2 != 0 { // 8-byte texels at an even word offset
				t.texels = append(t.texels, 0)
			}
			r.texel_offset = C.uint32_t(len(t.texels))
			for y := 0; y < b.Dy(); y++ {
				for x := 0; x < b.Dx(); x++ {
					t.putRGBA16(v.img.At(x, y).RGBA())
				}
			}
			// The border texel: what At returns outside the bounds (u == 1, v == 0, NaN) —
			// color.YCbCr{} = (0, 34678, 0) for jpeg.Decode's *image.YCbCr, 0 for *image.RGBA.
			t.putRGBA16(v.img.At(b.Max.X, b.Min.Y).RGBA())
		} else {
			r.width = C.uint32_t(max(b.Dx(), 0)) // Dy() <= 0: the debug colour (0, 1, 1), no texels
		}
	case *NoiseTexture: // RTX_NOISE_TEXELS: gradients (float32 bits), then permX, permY, permZ
		r._type, r.scale = C.RTX_TEX_NOISE, C.float(v.scale)
		r.texel_offset = C.uint32_t(len(t.texels))
		for _, g := range v.perlin.randVec3 {
			for _, c := range [3]float32{g.X, g.Y, g.Z} {
				t.texels = append(t.texels, C.uint32_t(math.Float32bits(c)))
			}
		}
		for _, perm := range [][]int{v.perlin.permX, v.perlin.permY, v.perlin.permZ} {
			for _, p := range perm {
				t.texels = append(t.texels, C.uint32_t(p))
			}
		}
	default:
		return 0, errUnsupported
	}
	i := C.uint32_t(len(t.textures))
	t.textures = append(t.textures, r)
	t.texIdx[tex] = i
	return i, nil
}

func (t *gpuTables) material(m Material) (C.uint32_t, error) {
	if i, ok := t.matIdx[m]; ok {
		return i, nil
	}
	var r C.rtx_material
	switch v := m.(type) {
	case *Lambertian:
		ti, err := t.texture(v.albedo)
		if err != nil {
			return 0, err
		}
		r._type, r.texture = C.RTX_MAT_LAMBERTIAN, ti
	case *Metal:
		r._type, r.fuzz, r.albedo = C.RTX_MAT_METAL, C.float(v.fuzz), vec(v.albedo.GetColor())
	case *Dielectric:
		r._type, r.ior = C.RTX_MAT_DIELECTRIC, C.float(v.refractiveIndex)
	case DiffuseLight, *DiffuseLight:
		d, ok := v.(DiffuseLight)
		if !ok {
			d = *v.(*DiffuseLight)
		}
		ti, err := t.texture(d.emit)
		if err != nil {
			return 0, err
		}
		r._type, r.texture = C.RTX_MAT_DIFFUSE_LIGHT, ti
	default:
		return 0, errUnsupported
	}
	i := C.uint32_t(len(t.materials))
	t.materials = append(t.materials, r)
	t.materialOf = append(t.materialOf, m)
	t.matIdx[m] = i
	return i, nil
}

// ref walks the tree in pre-order (a node before its children, left before right), the
// order NewBVH (bvh.go:142-185) creates it in.
func (t *gpuTables) ref(h Hittable) (C.int32_t, error) {
	switch v := h.(type) {
	case *BVH:
		me := len(t.nodes)
		b := v.bBox
		t.nodes = append(t.nodes, C.rtx_bvh_node{
			bmin: [3]C.float{C.float(b.x.min), C.float(b.y.min), C.float(b.z.min)},
			bmax: [3]C.float{C.float(b.x.max), C.float(b.y.max), C.float(b.z.max)},
		})
		l, err := t.ref(v.left)
		if err != nil {
			return 0, err
		}
		r := l
		if v.right != v.left { // one-element split: left == right (bvh.go:162-165)
			if r, err = t.ref(v.right); err != nil {
				return 0, err
			}
		}
		t.nodes[me].left, t.nodes[me].right = l, r
		return C.int32_t(me), nil
	case *Sphere:
		mi, err := t.material(v.Material)
		if err != nil {
			return 0, err
		}
		t.spheres = append(t.spheres, C.rtx_sphere{center: vec(v.Center), radius: C.float(v.Radius), material: mi})
		t.sphereOf = append(t.sphereOf, v)
		return primRef(C.RTX_PRIM_SPHERE, len(t.spheres)-1), nil
	case Quad, *Quad: // fields as NewQuad derived them (hittables.go:149-165)
		q, ok := v.(Quad)
		if !ok {
			q = *v.(*Quad)
		}
		mi, err := t.material(q.material)
		if err != nil {
			return 0, err
		}
		t.quads = append(t.quads, C.rtx_quad{
			q: vec(q.Q), material: mi, u: vec(q.u), d: C.float(q.D), v: vec(q.v), w: vec(q.w), normal: vec(q.normal),
		})
		t.quadOf = append(t.quadOf, q)
		return primRef(C.RTX_PRIM_QUAD, len(t.quads)-1), nil
	case *World: // a World nested in the tree (hittables.go:55-72 as a BVH child): a list ref
		// (an empty one is a miss: a list of no items, ABI 6)
		refs := make([]C.int32_t, len(v.hittables))
		for i, h := range v.hittables {
			r, err := t.ref(h)
			if err != nil {
				return 0, err
			}
			refs[i] = r
		}
		first := len(t.listRefs)
		t.listRefs = append(t.listRefs, refs...)
		t.lists = append(t.lists, C.rtx_list{first: C.uint32_t(first), count: C.uint32_t(len(refs))})
		return primRef(C.RTX_PRIM_LIST, len(t.lists)-1), nil
	default:
		return 0, errUnsupported
	}
}

// rtxError is a library error code with rtx_last_error's message (Render's error return).
type rtxError struct {
	code C.int
	msg  string
}

func (e *rtxError) Error() string { return fmt.Sprintf("rtx error %d: %s", int(e.code), e.msg) }

func rtxErr(rc C.int) error { return &rtxError{code: rc, msg: C.GoString(C.rtx_last_error())} }

// gpuMissing: the library cannot run this render at all (no device, a feature it reports as
// unsupported): RenderGPU then renders on the CPU.  (RCCL trouble is not among them: rtx_render
// assembles the bands with per-band copies when RCCL is unavailable or fails, rtx.h.)
func gpuMissing(rc C.int) bool {
	return rc == C.RTX_ERR_UNSUPPORTED || rc == C.RTX_ERR_NO_DEVICE || rc == C.RTX_ERR_RCCL
}

// flatten: the tree Render receives as rtx.h tables; a plain *World gives one root per item
// (its linear closest-hit scan, hittables.go:55-72).
func flatten(world Hittable) (*gpuTables, error) {
	t := &gpuTables{matIdx: map[Material]C.uint32_t{}, texIdx: map[Texture]C.uint32_t{}}
	items := []Hittable{world}
	if wl, ok := world.(*World); ok {
		items = wl.hittables
	}
	for _, it := range items {
		r, err := t.ref(it)
		if err != nil {
			return nil, err
		}
		t.roots = append(t.roots, r)
	}
	if len(t.roots) == 0 || len(t.materials) == 0 {
		return nil, errUnsupported
	}
	return t, nil
}

// errFallback: the GPU path cannot carry this render (a scene part it does not flatten, no
// device, a feature the library reports unsupported): the CPU path renders it instead.
var errFallback = errors.New("rtx: render on the CPU path")

// renderGPU is the hook at the top of Render (camera.go:180, INTEGRATION.md): with WithGPUs(n > 0)
// (or RTX_GPUS) it renders on the devices and reports done; otherwise, or when the GPU path cannot
// carry the render, Render continues on its CPU path.
func (c *Camera) renderGPU(world Hittable, writer io.Writer) (bool, error) {
	cfg := c.gpuConfig()
	if cfg.gpus <= 0 || cfg.fallback.Load() {
		return false, nil
	}
	err := c.renderOnDevices(world, writer, cfg.seed, cfg.gpus)
	if errors.Is(err, errFallback) {
		return false, nil
	}
	return true, err
}

// RenderGPU is Render (camera.go:180) on the MI355X path with an explicit seed and device count,
// whatever the camera's options: same P3 bytes to writer, same error return; the CPU Render for
// anything the GPU path does not carry.
func (c *Camera) RenderGPU(world Hittable, writer io.Writer, seed uint64, gpus int) error {
	err := c.renderOnDevices(world, writer, seed, max(gpus, 1))
	if errors.Is(err, errFallback) {
		cfg := c.gpuConfig()
		cfg.fallback.Store(true)
		defer cfg.fallback.Store(false)
		return c.Render(world, writer)
	}
	return err
}

// sceneOf uploads the world once (rtx_scene_create, or rtx_scene_create_spheres /
// rtx_scene_create_world for a NewBVHFromWorldGPU tree): the caller destroys the scene.  Go slices
// stay pinned only for the call; librtx copies them and keeps no pointer into Go memory.
func sceneOf(world Hittable, seed uint64) (*C.rtx_scene, error) {
	scene, _, err := sceneTables(world, seed)
	return scene, err
}

// sceneTables is sceneOf that also returns the flattened tables (HitBatch maps hits back through them).
func sceneTables(world Hittable, seed uint64) (*C.rtx_scene, *gpuTables, error) {
	var pin runtime.Pinner
	defer pin.Unpin()
	var scene *C.rtx_scene
	if g, ok := world.(*gpuBVH); ok {
		t := &gpuTables{matIdx: map[Material]C.uint32_t{}, texIdx: map[Texture]C.uint32_t{}}
		// the World's list in Add order, NewBVH's input: spheres and quads, each numbered in Add order among its
		// kind (HitBatch's sphereOf / quadOf are these tables); anything else keeps the CPU path
		var items []C.int32_t
		for _, h := range g.world.hittables {
			switch v := h.(type) {
			case *Sphere:
				mi, err := t.material(v.Material)
				if err != nil {
					return nil, nil, err
				}
				t.spheres = append(t.spheres, C.rtx_sphere{center: vec(v.Center), radius: C.float(v.Radius), material: mi})
				t.sphereOf = append(t.sphereOf, v)
				items = append(items, primRef(C.RTX_PRIM_SPHERE, len(t.spheres)-1))
			case Quad, *Quad: // fields as NewQuad derived them (hittables.go:149-165)
				q, ok := v.(Quad)
				if !ok {
					q = *v.(*Quad)
				}
				mi, err := t.material(q.material)
				if err != nil {
					return nil, nil, err
				}
				t.quads = append(t.quads, C.rtx_quad{
					q: vec(q.Q), material: mi, u: vec(q.u), d: C.float(q.D), v: vec(q.v), w: vec(q.w), normal: vec(q.normal),
				})
				t.quadOf = append(t.quadOf, q)
				items = append(items, primRef(C.RTX_PRIM_QUAD, len(t.quads)-1))
			default:
				return nil, nil, errFallback
			}
		}
		if len(items) == 0 {
			return nil, nil, errFallback
		}
		pin.Pin(&t.materials[0])
		var tex *C.rtx_texture
		var texels *C.uint32_t
		if len(t.textures) > 0 {
			pin.Pin(&t.textures[0])
			tex = &t.textures[0]
		}
		if len(t.texels) > 0 {
			pin.Pin(&t.texels[0])
			texels = &t.texels[0]
		}
		if len(t.quads) == 0 { // a World of spheres: the table in order is the list
			pin.Pin(&t.spheres[0])
			if rc := C.rtx_scene_create_spheres(&t.spheres[0], C.uint32_t(len(t.spheres)), &t.materials[0],
				C.uint32_t(len(t.materials)), tex, C.uint32_t(len(t.textures)), texels, C.uint64_t(len(t.texels)),
				C.uint64_t(seed), 0, &scene, nil); rc != 0 {
				return nil, nil, rtxErr(rc)
			}
			return scene, t, nil
		}
		var sph *C.rtx_sphere
		if len(t.spheres) > 0 {
			pin.Pin(&t.spheres[0])
			sph = &t.spheres[0]
		}
		pin.Pin(&items[0])
		pin.Pin(&t.quads[0])
		if rc := C.rtx_scene_create_world(&items[0], C.uint32_t(len(items)), sph, C.uint32_t(len(t.spheres)),
			&t.quads[0], C.uint32_t(len(t.quads)), &t.materials[0], C.uint32_t(len(t.materials)), tex,
			C.uint32_t(len(t.textures)), texels, C.uint64_t(len(t.texels)), C.uint64_t(seed), 0, &scene, nil); rc != 0 {
			return nil, nil, rtxErr(rc)
		}
		return scene, t, nil
	}
	t, err := flatten(world)
	if err != nil {
		return nil, nil, err
	}
	var desc C.rtx_scene_desc
	if len(t.nodes) > 0 {
		pin.Pin(&t.nodes[0])
		desc.nodes, desc.n_nodes = &t.nodes[0], C.uint32_t(len(t.nodes))
	}
	pin.Pin(&t.roots[0])
	desc.roots, desc.n_roots = &t.roots[0], C.uint32_t(len(t.roots))
	if len(t.spheres) > 0 {
		pin.Pin(&t.spheres[0])
		desc.spheres, desc.n_spheres = &t.spheres[0], C.uint32_t(len(t.spheres))
	}
	if len(t.quads) > 0 {
		pin.Pin(&t.quads[0])
		desc.quads, desc.n_quads = &t.quads[0], C.uint32_t(len(t.quads))
	}
	pin.Pin(&t.materials[0])
	desc.materials, desc.n_materials = &t.materials[0], C.uint32_t(len(t.materials))
	if len(t.textures) > 0 {
		pin.Pin(&t.textures[0])
		desc.textures, desc.n_textures = &t.textures[0], C.uint32_t(len(t.textures))
	}
	if len(t.texels) > 0 {
		pin.Pin(&t.texels[0])
		desc.texels, desc.n_texels = &t.texels[0], C.uint64_t(len(t.texels))
	}
	if len(t.lists) > 0 {
		pin.Pin(&t.lists[0])
		desc.lists, desc.n_lists = &t.lists[0], C.uint32_t(len(t.lists))
	}
	if len(t.listRefs) > 0 {
		pin.Pin(&t.listRefs[0])
		desc.list_refs, desc.n_list_refs = &t.listRefs[0], C.uint32_t(len(t.listRefs))
	}
	if rc := C.rtx_scene_create(&desc, &scene); rc != 0 {
		return nil, nil, rtxErr(rc)
	}
	return scene, t, nil
}

// HitBatch is Hittable.Hit (hittables.go:7-20) for a batch of rays on the GPU: hits[i], ok[i] are what
// world.Hit(&rays[i], rayT[i]) returns (rtx_trace, rtx.h "ray queries": the closest hit with the ray's own
// interval, ties as the reference's walk resolves them).  The world is flattened and uploaded for the call
// (sceneOf) and rtx_hit.prim / .material are mapped back to the Go values that were flattened: the hit's
// Material is the primitive's own.  u and v are filled (RTX_TRACE_UV).  A world the GPU path does not carry
// returns errFallback; the caller then loops over world.Hit.
func HitBatch(world Hittable, rays []Ray, rayT []Interval) ([]HitInfo, []bool, error) {
	if len(rays) != len(rayT) {
		return nil, nil, errors.New("rtx: HitBatch needs one interval per ray")
	}
	infos, oks := make([]HitInfo, len(rays)), make([]bool, len(rays))
	if len(rays) == 0 {
		return infos, oks, nil
	}
	scene, t, err := sceneTables(world, 0)
	if errors.Is(err, errUnsupported) {
		return nil, nil, errFallback
	}
	if err != nil {
		return nil, nil, err
	}
	defer C.rtx_scene_destroy(scene)
	// rtx_trace wants both tables 16-B aligned, which a Go slice of a 4-B aligned struct does not promise: byte
	// slices with room to start on a 16-B boundary, pinned for the call (they hold no Go pointers)
	aligned := func(bytes uintptr) ([]byte, unsafe.Pointer) {
		buf := make([]byte, bytes+16)
		off := (16 - uintptr(unsafe.Pointer(&buf[0]))%16) % 16
		return buf, unsafe.Pointer(&buf[off])
	}
	inBuf, inPtr := aligned(uintptr(len(rays)) * unsafe.Sizeof(C.rtx_ray{}))
	outBuf, outPtr := aligned(uintptr(len(rays)) * unsafe.Sizeof(C.rtx_hit{}))
	var pin runtime.Pinner
	defer pin.Unpin()
	pin.Pin(&inBuf[0])
	pin.Pin(&outBuf[0])
	in, out := (*C.rtx_ray)(inPtr), (*C.rtx_hit)(outPtr)
	cin, cout := unsafe.Slice(in, len(rays)), unsafe.Slice(out, len(rays))
	for i := range rays {
		cin[i] = C.rtx_ray{origin: vec(rays[i].origin), tmin: C.float(rayT[i].min), dir: vec(rays[i].dir), tmax: C.float(rayT[i].max)}
	}
	if rc := C.rtx_trace(scene, in, C.uint64_t(len(rays)), out, C.RTX_TRACE_UV, nil); rc != 0 {
		if gpuMissing(rc) {
			return nil, nil, errFallback
		}
		return nil, nil, rtxErr(rc)
	}
	v3 := func(a [3]C.float) Vec3 { return NewVec3(float32(a[0]), float32(a[1]), float32(a[2])) }
	for i := range cout {
		var rec C.rtx_hit = cout[i]
		if rec.prim == C.RTX_HIT_NONE {
			continue
		}
		var mat Material
		switch idx := int(rec.prim & 0x0FFFFFFF); rec.prim >> 28 {
		case C.RTX_PRIM_SPHERE:
			mat = t.sphereOf[idx].Material
		case C.RTX_PRIM_QUAD:
			mat = t.quadOf[idx].material
		}
		if mat == nil { // (cannot happen: prim names a flattened primitive)
			mat = t.materialOf[int(rec.material)]
		}
		infos[i] = HitInfo{point: v3(rec.point), normal: v3(rec.normal), t: float32(rec.t), u: float32(rec.u),
			v: float32(rec.v), material: mat, frontFace: rec.front_face != 0}
		oks[i] = true
	}
	return infos, oks, nil
}

// PathKey names the Philox blocks of one path event (rtx_path_key, rtx.h "path building blocks"): the global
// pixel index, the sample, and the event (0 = GetRay, s + 1 = the scatter after segment s).  Draws is what
// RayBatch reports: the rand.Float32() calls GetRay made.
type PathKey struct {
	Pixel, Sample, Event, Draws uint32
}

// Bounce is Material.Emit and Material.Scatter of one hit (rtx_bounce): Ray is ScatterInfo's ray, to be hit
// with GetColor's Interval{0.001, +Inf}; Draws counts the rand.Float32() calls Scatter made.
type Bounce struct {
	Scattered, Emits     bool
	Attenuation, Emitted Vec3
	Ray                  Ray
	Draws                uint32
}

// alignedBytes is a byte slice with room to start on a 16-B boundary, which rtx_trace, rtx_camera_rays and
// rtx_shade want of every table and a Go slice of a 4-B aligned struct does not promise.  The caller pins
// &buf[0] for the call (the bytes hold no Go pointers).
func alignedBytes(bytes uintptr) ([]byte, unsafe.Pointer) {
	buf := make([]byte, bytes+16)
	off := (16 - uintptr(unsafe.Pointer(&buf[0]))%16) % 16
	return buf, unsafe.Pointer(&buf[off])
}

// RayBatch is GetRay (camera.go:265-299) for samples [firstSample, firstSample + count) of every pixel on the
// GPU (rtx_camera_rays): ray (k - firstSample) * W * H + y * W + x is the ray of pixel (x, y) and sample k under
// the RNG contract's seed, and keys[i] is the key of its first scatter (Event 1).  Every ray is to be hit with
// Interval{0.001, +Inf}.
func (c *Camera) RayBatch(seed uint64, firstSample, count uint32) ([]Ray, []PathKey, error) {
	c.init()
	cam := c.gpuCamera()
	region := C.rtx_region{x0: 0, y0: 0, width: cam.image_width, height: cam.image_height, rank: 0, world: 1, stripe: 0}
	n := int(count) * int(cam.image_width) * int(cam.image_height)
	rays, keys := make([]Ray, n), make([]PathKey, n)
	if n == 0 {
		return rays, keys, nil
	}
	rayBuf, rayPtr := alignedBytes(uintptr(n) * unsafe.Sizeof(C.rtx_ray{}))
	keyBuf, keyPtr := alignedBytes(uintptr(n) * unsafe.Sizeof(C.rtx_path_key{}))
	var pin runtime.Pinner
	defer pin.Unpin()
	pin.Pin(&rayBuf[0])
	pin.Pin(&keyBuf[0])
	outRays, outKeys := (*C.rtx_ray)(rayPtr), (*C.rtx_path_key)(keyPtr)
	if rc := C.rtx_camera_rays(&cam, C.uint64_t(seed), &region, C.uint32_t(firstSample), C.uint32_t(count), outRays, outKeys); rc != 0 {
		if gpuMissing(rc) {
			return nil, nil, errFallback
		}
		return nil, nil, rtxErr(rc)
	}
	v3 := func(a [3]C.float) Vec3 { return NewVec3(float32(a[0]), float32(a[1]), float32(a[2])) }
	crays, ckeys := unsafe.Slice(outRays, n), unsafe.Slice(outKeys, n)
	for i := range rays {
		var r C.rtx_ray = crays[i]
		var k C.rtx_path_key = ckeys[i]
		rays[i] = Ray{origin: v3(r.origin), dir: v3(r.dir)}
		keys[i] = PathKey{Pixel: uint32(k.pixel), Sample: uint32(k.sample), Event: uint32(k.event), Draws: uint32(k.draws)}
	}
	return rays, keys, nil
}

// ScatterBatch is hit.material.Emit and hit.material.Scatter (ray.go:41-42) for a batch on the GPU (rtx_shade):
// rays[i] is the ray that was hit, hits[i] its HitInfo as HitBatch returned it (a nil material: no hit, an all-zero
// Bounce), keys[i] the path event whose Philox blocks the scatter draws from, seed the RNG contract's seed.  The
// world is flattened and uploaded for the call, as in HitBatch.
func ScatterBatch(world Hittable, rays []Ray, hits []HitInfo, keys []PathKey, seed uint64) ([]Bounce, error) {
	if len(rays) != len(hits) || len(rays) != len(keys) {
		return nil, errors.New("rtx: ScatterBatch needs one hit and one key per ray")
	}
	out := make([]Bounce, len(rays))
	if len(rays) == 0 {
		return out, nil
	}
	scene, t, err := sceneTables(world, 0)
	if errors.Is(err, errUnsupported) {
		return nil, errFallback
	}
	if err != nil {
		return nil, err
	}
	defer C.rtx_scene_destroy(scene)
	n := uintptr(len(rays))
	rayBuf, rayPtr := alignedBytes(n * unsafe.Sizeof(C.rtx_ray{}))
	hitBuf, hitPtr := alignedBytes(n * unsafe.Sizeof(C.rtx_hit{}))
	keyBuf, keyPtr := alignedBytes(n * unsafe.Sizeof(C.rtx_path_key{}))
	outBuf, outPtr := alignedBytes(n * unsafe.Sizeof(C.rtx_bounce{}))
	var pin runtime.Pinner
	defer pin.Unpin()
	pin.Pin(&rayBuf[0])
	pin.Pin(&hitBuf[0])
	pin.Pin(&keyBuf[0])
	pin.Pin(&outBuf[0])
	inRays, inHits, inKeys, bounces := (*C.rtx_ray)(rayPtr), (*C.rtx_hit)(hitPtr), (*C.rtx_path_key)(keyPtr), (*C.rtx_bounce)(outPtr)
	crays, chits, ckeys := unsafe.Slice(inRays, len(rays)), unsafe.Slice(inHits, len(rays)), unsafe.Slice(inKeys, len(rays))
	for i := range rays {
		crays[i] = C.rtx_ray{origin: vec(rays[i].origin), tmin: 0.001, dir: vec(rays[i].dir), tmax: C.float(math.Inf(1))}
		ckeys[i] = C.rtx_path_key{pixel: C.uint32_t(keys[i].Pixel), sample: C.uint32_t(keys[i].Sample), event: C.uint32_t(keys[i].Event)}
		chits[i] = C.rtx_hit{t: C.float(math.Inf(1)), prim: C.RTX_HIT_NONE}
		mi, known := t.matIdx[hits[i].material]
		if hits[i].material == nil || !known {
			continue
		}
		front := C.uint32_t(0)
		if hits[i].frontFace {
			front = 1
		}
		// (prim only says "a hit" to rtx_shade: the material index is what it reads)
		chits[i] = C.rtx_hit{t: C.float(hits[i].t), prim: 0, material: mi, front_face: front, point: vec(hits[i].point),
			u: C.float(hits[i].u), normal: vec(hits[i].normal), v: C.float(hits[i].v)}
	}
	if rc := C.rtx_shade(scene, C.uint64_t(seed), inRays, inHits, inKeys, C.uint64_t(len(rays)), bounces, 0, nil); rc != 0 {
		if gpuMissing(rc) {
			return nil, errFallback
		}
		return nil, rtxErr(rc)
	}
	v3 := func(a [3]C.float) Vec3 { return NewVec3(float32(a[0]), float32(a[1]), float32(a[2])) }
	for i, rec := range unsafe.Slice(bounces, len(rays)) {
		var b C.rtx_bounce = rec
		out[i] = Bounce{Scattered: b.flags&C.RTX_BOUNCE_SCATTERED != 0, Emits: b.flags&C.RTX_BOUNCE_EMITS != 0,
			Attenuation: v3(b.attenuation), Emitted: v3(b.emitted), Draws: uint32(b.rng_draws),
			Ray: Ray{origin: v3(b.ray.origin), dir: v3(b.ray.dir)}}
	}
	return out, nil
}

// Light is one row of the emitter table (rtx_light, rtx.h "direct light sampling"): Quad says which table Index
// names (the flattener's sphere or quad numbering), Area is the float32 area the light sample divides by.
type Light struct {
	Quad  bool
	Index uint32
	Area  float32
}

// Lights is the emitter table of a world (rtx_scene_lights): its referenced DiffuseLight spheres, then quads.  The
// world is flattened and uploaded for the call, as in HitBatch (rtx_lights answers from a description alone).
func Lights(world Hittable) ([]Light, error) {
	scene, _, err := sceneTables(world, 0)
	if errors.Is(err, errUnsupported) {
		return nil, errFallback
	}
	if err != nil {
		return nil, err
	}
	defer C.rtx_scene_destroy(scene)
	var n C.uint32_t
	if rc := C.rtx_scene_lights(scene, nil, 0, &n); rc != 0 {
		return nil, rtxErr(rc)
	}
	out := make([]Light, int(n))
	if n == 0 {
		return out, nil
	}
	tab := make([]C.rtx_light, int(n))
	if rc := C.rtx_scene_lights(scene, &tab[0], n, &n); rc != 0 {
		return nil, rtxErr(rc)
	}
	for i := range out {
		var l C.rtx_light = tab[i]
		out[i] = Light{Quad: uint32(l.prim)>>28 == C.RTX_PRIM_QUAD, Index: uint32(l.prim) & 0x0FFFFFFF, Area: float32(l.area)}
	}
	return out, nil
}

// DirectSample is one light sample at a Lambertian hit and its shadow ray's answer (rtx_direct_sample): Radiance is
// (albedo * emitted) * Geom WITHOUT the visibility, which the caller applies: L += T * Radiance when Visible.
type DirectSample struct {
	Sampled, Visible bool
	Radiance         Vec3
	Shadow           Ray // to be hit with Interval{0.001, 0.999}
	Light, Draws     uint32
	Geom             float32
}

// DirectBatch samples one emitter point per hit and walks the shadow ray to it on the GPU (rtx_direct): hits[i] as
// HitBatch returned it, keys[i] the key of the scatter at that hit, seed the RNG contract's seed.  The world is
// flattened and uploaded for the call, as in HitBatch.
func DirectBatch(world Hittable, hits []HitInfo, keys []PathKey, seed uint64) ([]DirectSample, error) {
	if len(hits) != len(keys) {
		return nil, errors.New("rtx: DirectBatch needs one key per hit")
	}
	out := make([]DirectSample, len(hits))
	if len(hits) == 0 {
		return out, nil
	}
	scene, t, err := sceneTables(world, 0)
	if errors.Is(err, errUnsupported) {
		return nil, errFallback
	}
	if err != nil {
		return nil, err
	}
	defer C.rtx_scene_destroy(scene)
	n := uintptr(len(hits))
	hitBuf, hitPtr := alignedBytes(n * unsafe.Sizeof(C.rtx_hit{}))
	keyBuf, keyPtr := alignedBytes(n * unsafe.Sizeof(C.rtx_path_key{}))
	outBuf, outPtr := alignedBytes(n * unsafe.Sizeof(C.rtx_direct_sample{}))
	var pin runtime.Pinner
	defer pin.Unpin()
	pin.Pin(&hitBuf[0])
	pin.Pin(&keyBuf[0])
	pin.Pin(&outBuf[0])
	inHits, inKeys, samples := (*C.rtx_hit)(hitPtr), (*C.rtx_path_key)(keyPtr), (*C.rtx_direct_sample)(outPtr)
	chits, ckeys := unsafe.Slice(inHits, len(hits)), unsafe.Slice(inKeys, len(hits))
	for i := range hits {
		ckeys[i] = C.rtx_path_key{pixel: C.uint32_t(keys[i].Pixel), sample: C.uint32_t(keys[i].Sample), event: C.uint32_t(keys[i].Event)}
		chits[i] = C.rtx_hit{t: C.float(math.Inf(1)), prim: C.RTX_HIT_NONE}
		mi, known := t.matIdx[hits[i].material]
		if hits[i].material == nil || !known {
			continue
		}
		front := C.uint32_t(0)
		if hits[i].frontFace {
			front = 1
		}
		// (prim only says "a hit" to rtx_direct: the material index, the point and the normal are what it reads)
		chits[i] = C.rtx_hit{t: C.float(hits[i].t), prim: 0, material: mi, front_face: front, point: vec(hits[i].point),
			u: C.float(hits[i].u), normal: vec(hits[i].normal), v: C.float(hits[i].v)}
	}
	if rc := C.rtx_direct(scene, C.uint64_t(seed), inHits, inKeys, C.uint64_t(len(hits)), samples, 0, nil); rc != 0 {
		if gpuMissing(rc) {
			return nil, errFallback
		}
		return nil, rtxErr(rc)
	}
	v3 := func(a [3]C.float) Vec3 { return NewVec3(float32(a[0]), float32(a[1]), float32(a[2])) }
	for i, rec := range unsafe.Slice(samples, len(hits)) {
		var d C.rtx_direct_sample = rec
		out[i] = DirectSample{Sampled: d.flags&C.RTX_DIRECT_SAMPLED != 0, Visible: d.flags&C.RTX_DIRECT_VISIBLE != 0,
			Radiance: v3(d.radiance), Shadow: Ray{origin: v3(d.ray.origin), dir: v3(d.ray.dir)},
			Light: uint32(d.light), Draws: uint32(d.rng_draws), Geom: float32(d.geom)}
	}
	return out, nil
}

// EmitterWeight is the power-heuristic weight of a bounce that found an emitter (rtx_emitter_weight_record, rtx.h
// "multiple importance sampling of the direct light"): the emission the bounce adds is Emitted * Weight, and the light
// sample at the hit the bounce left is weighted 1 / (1 + Geom*Geom) of its own DirectSample.Geom.  Weighted false:
// Weight is 1 (nothing to share the emitter point with) and Geom 0.  Light is the emitter table's index of the
// primitive found, or NoLight.
type EmitterWeight struct {
	Weighted     bool
	Weight, Geom float32
	Light        uint32
}

// NoLight is EmitterWeight.Light of a primitive the emitter table does not hold (RTX_LIGHT_NONE).
const NoLight = uint32(C.RTX_LIGHT_NONE)

// EmitterWeights traces bounces[i] (with GetColor's Interval{0.001, +Inf}) on the GPU and weights what it found
// against a light sample at from[i], the Lambertian hit the bounce left (rtx_trace, then rtx_emitter_weight).  HitInfo
// does not name its primitive, which the weight's area lookup needs: hence the trace here, not a slice of hits.  The
// world is flattened and uploaded for the call, as in HitBatch.
func EmitterWeights(world Hittable, from []HitInfo, bounces []Ray) ([]EmitterWeight, error) {
	if len(from) != len(bounces) {
		return nil, errors.New("rtx: EmitterWeights needs one bounce ray per hit")
	}
	out := make([]EmitterWeight, len(from))
	if len(from) == 0 {
		return out, nil
	}
	scene, t, err := sceneTables(world, 0)
	if errors.Is(err, errUnsupported) {
		return nil, errFallback
	}
	if err != nil {
		return nil, err
	}
	defer C.rtx_scene_destroy(scene)
	n := uintptr(len(from))
	rayBuf, rayPtr := alignedBytes(n * unsafe.Sizeof(C.rtx_ray{}))
	fromBuf, fromPtr := alignedBytes(n * unsafe.Sizeof(C.rtx_hit{}))
	hitBuf, hitPtr := alignedBytes(n * unsafe.Sizeof(C.rtx_hit{}))
	outBuf, outPtr := alignedBytes(n * unsafe.Sizeof(C.rtx_emitter_weight_record{}))
	var pin runtime.Pinner
	defer pin.Unpin()
	pin.Pin(&rayBuf[0])
	pin.Pin(&fromBuf[0])
	pin.Pin(&hitBuf[0])
	pin.Pin(&outBuf[0])
	inRays, inFrom, found := (*C.rtx_ray)(rayPtr), (*C.rtx_hit)(fromPtr), (*C.rtx_hit)(hitPtr)
	weights := (*C.rtx_emitter_weight_record)(outPtr)
	crays, cfrom := unsafe.Slice(inRays, len(from)), unsafe.Slice(inFrom, len(from))
	for i := range from {
		crays[i] = C.rtx_ray{origin: vec(bounces[i].origin), tmin: 0.001, dir: vec(bounces[i].dir), tmax: C.float(math.Inf(1))}
		cfrom[i] = C.rtx_hit{t: C.float(math.Inf(1)), prim: C.RTX_HIT_NONE}
		mi, known := t.matIdx[from[i].material]
		if from[i].material == nil || !known {
			continue
		}
		// (prim only says "a hit" for the hit a bounce left: its material, point and normal are what the weight reads)
		cfrom[i] = C.rtx_hit{t: C.float(from[i].t), prim: 0, material: mi, point: vec(from[i].point), normal: vec(from[i].normal)}
	}
	if rc := C.rtx_trace(scene, inRays, C.uint64_t(len(from)), found, 0, nil); rc != 0 {
		if gpuMissing(rc) {
			return nil, errFallback
		}
		return nil, rtxErr(rc)
	}
	if rc := C.rtx_emitter_weight(scene, inFrom, found, C.uint64_t(len(from)), weights, 0, nil); rc != 0 {
		return nil, rtxErr(rc)
	}
	for i, rec := range unsafe.Slice(weights, len(from)) {
		var w C.rtx_emitter_weight_record = rec
		out[i] = EmitterWeight{Weighted: w.flags&C.RTX_EMITTER_WEIGHTED != 0, Weight: float32(w.weight), Geom: float32(w.geom),
			Light: uint32(w.light)}
	}
	return out, nil
}

// gpuCamera is Camera.init's derived state (camera.go:128-165) as rtx.h's kernel constants.
func (c *Camera) gpuCamera() C.rtx_camera {
	return C.rtx_camera{
		image_width: C.uint32_t(c.imageWidth), image_height: C.uint32_t(c.imageHeight),
		samples_per_pixel: C.uint32_t(c.samplesPerPixel), max_depth: C.uint32_t(max(c.bounceDepth, 0)),
		center: vec(c.center), defocus_angle: C.float(c.defocusAngleRadians),
		pixel00: vec(c.pixel00), pixel_du: vec(c.pixelDu), pixel_dv: vec(c.pixelDv),
		defocus_disk_u: vec(c.defocusDiskU), defocus_disk_v: vec(c.defocusDiskV),
		background: vec(c.background.GetColor()),
	}
}

// RenderProgressive is Render on one MI355X in passes of passSamples samples per pixel (rtx_accum,
// rtx.h "progressive rendering"): after every pass onPass (when not nil) is told the samples done
// and the pixels still noisy at WithNoiseTolerance's tolerance, and returning false stops the render
// there.  It ends at samplesPerPixel, when onPass says so, or, with WithNoiseTolerance, when no pixel
// is noisy, and writes the P3 bytes of the image so far: after n samples exactly the bytes a Render
// with samplesPerPixel = n writes.  onPass runs between two C calls, on the caller's goroutine: no C
// code calls back into Go.  A scene the GPU path does not carry is an error here (there is no CPU
// path that stops early).
func (c *Camera) RenderProgressive(world Hittable, writer io.Writer, passSamples int, onPass func(done int, noisy uint64) bool) error {
	c.init()
	cfg := c.gpuConfig()
	if passSamples <= 0 {
		passSamples = c.samplesPerPixel
	}
	scene, err := sceneOf(world, cfg.seed)
	if err != nil {
		return err
	}
	defer C.rtx_scene_destroy(scene) // (deferred calls run last in, first out: the accumulator goes first)
	cam := c.gpuCamera()
	region := C.rtx_region{x0: 0, y0: 0, width: cam.image_width, height: cam.image_height, rank: 0, world: 1, stripe: 0}
	var acc *C.rtx_accum
	if rc := C.rtx_accum_create(scene, &cam, C.uint64_t(cfg.seed), &region, &acc); rc != 0 {
		return rtxErr(rc)
	}
	defer C.rtx_accum_destroy(acc)
	for done := 0; done < c.samplesPerPixel; {
		count := min(passSamples, c.samplesPerPixel-done)
		// the default stream orders the passes and the resolves of this accumulator
		if rc := C.rtx_accum_add(acc, C.uint32_t(count), nil, 0, nil); rc != 0 {
			return rtxErr(rc)
		}
		done = int(C.rtx_accum_samples(acc))
		if onPass == nil && cfg.noiseTol <= 0 {
			continue // nobody looks at the image before the end: the passes stay enqueued back to back
		}
		var noisy C.uint64_t
		if rc := C.rtx_accum_resolve(acc, nil, nil, C.float(cfg.noiseTol), &noisy); rc != 0 {
			return rtxErr(rc)
		}
		if onPass != nil && !onPass(done, uint64(noisy)) {
			break
		}
		if cfg.noiseTol > 0 && noisy == 0 {
			break
		}
	}
	text := make([]byte, int(C.rtx_ppm_max_bytes(cam.image_width, cam.image_height)))
	var n C.uint64_t
	if rc := C.rtx_accum_ppm(acc, (*C.char)(unsafe.Pointer(&text[0])), C.uint64_t(len(text)), &n); rc != 0 {
		return rtxErr(rc)
	}
	if rc := C.rtx_device_check(0); rc != 0 { // the passes ran without stats: the sticky error word, once
		return rtxErr(rc)
	}
	_, err = writer.Write(text[:int(n)])
	return err
}

// RenderDirect is Render with direct light sampling (rtx_accum_add_direct, rtx.h "direct light sampling"): every
// sample by the next-event estimator, in passes of passSamples (<= 0: one pass).  Same mean as Render, another image;
// a world without emitters gives Render's own image.
func (c *Camera) RenderDirect(world Hittable, writer io.Writer, passSamples int) error {
	return c.renderLightSampled(world, writer, passSamples, false)
}

// RenderMIS is RenderDirect with the light sample and the bounce weighted by the power heuristic (rtx_accum_add_mis,
// rtx.h "multiple importance sampling of the direct light"): same mean again, and no sample brighter than the
// emitter, however close a light lies to a surface.
func (c *Camera) RenderMIS(world Hittable, writer io.Writer, passSamples int) error {
	return c.renderLightSampled(world, writer, passSamples, true)
}

func (c *Camera) renderLightSampled(world Hittable, writer io.Writer, passSamples int, mis bool) error {
	c.init()
	cfg := c.gpuConfig()
	if passSamples <= 0 {
		passSamples = c.samplesPerPixel
	}
	scene, err := sceneOf(world, cfg.seed)
	if err != nil {
		return err
	}
	defer C.rtx_scene_destroy(scene) // (deferred calls run last in, first out: the accumulator goes first)
	cam := c.gpuCamera()
	region := C.rtx_region{x0: 0, y0: 0, width: cam.image_width, height: cam.image_height, rank: 0, world: 1, stripe: 0}
	var acc *C.rtx_accum
	if rc := C.rtx_accum_create(scene, &cam, C.uint64_t(cfg.seed), &region, &acc); rc != 0 {
		return rtxErr(rc)
	}
	defer C.rtx_accum_destroy(acc)
	for done := 0; done < c.samplesPerPixel; done = int(C.rtx_accum_samples(acc)) {
		count := min(passSamples, c.samplesPerPixel-done)
		rc := C.int(0)
		if mis {
			rc = C.rtx_accum_add_mis(acc, C.uint32_t(count), nil, 0, nil)
		} else {
			rc = C.rtx_accum_add_direct(acc, C.uint32_t(count), nil, 0, nil)
		}
		if rc != 0 {
			return rtxErr(rc)
		}
	}
	text := make([]byte, int(C.rtx_ppm_max_bytes(cam.image_width, cam.image_height)))
	var n C.uint64_t
	if rc := C.rtx_accum_ppm(acc, (*C.char)(unsafe.Pointer(&text[0])), C.uint64_t(len(text)), &n); rc != 0 {
		return rtxErr(rc)
	}
	if rc := C.rtx_device_check(0); rc != 0 {
		return rtxErr(rc)
	}
	_, err = writer.Write(text[:int(n)])
	return err
}

// RenderAdaptive is RenderProgressive with adaptive passes (rtx_accum_add_adaptive, rtx.h "adaptive sampling"): before
// every pass the 64-pixel tiles none of whose pixels is noisy at relTol are closed (once minSamples have been offered),
// and the pass samples the others only.  It ends when a pass found no open tile or at samplesPerPixel offered, and
// writes the P3 bytes of the image: every pixel the mean of the samples it received, bit for bit that pixel of a
// Render at as many samples.  onPass (when not nil) is told the samples offered and the tiles and pixels the pass
// sampled; returning false stops the render there.  Stopping on an estimate biases the image (a tile that has not seen
// its first bright sample closes early): minSamples is the guard.
func (c *Camera) RenderAdaptive(world Hittable, writer io.Writer, passSamples int, relTol float32, minSamples int, onPass func(offered int, openTiles, openPixels uint64) bool) error {
	c.init()
	cfg := c.gpuConfig()
	if passSamples <= 0 {
		passSamples = c.samplesPerPixel
	}
	scene, err := sceneOf(world, cfg.seed)
	if err != nil {
		return err
	}
	defer C.rtx_scene_destroy(scene)
	cam := c.gpuCamera()
	region := C.rtx_region{x0: 0, y0: 0, width: cam.image_width, height: cam.image_height, rank: 0, world: 1, stripe: 0}
	var acc *C.rtx_accum
	if rc := C.rtx_accum_create(scene, &cam, C.uint64_t(cfg.seed), &region, &acc); rc != 0 {
		return rtxErr(rc)
	}
	defer C.rtx_accum_destroy(acc)
	for offered := 0; offered < c.samplesPerPixel; {
		count := min(passSamples, c.samplesPerPixel-offered)
		var ad C.rtx_adapt_stats
		// the open-tile count is the stop signal, so every pass is waited for
		if rc := C.rtx_accum_add_adaptive(acc, C.uint32_t(count), C.float(relTol), C.uint32_t(max(minSamples, 0)), nil, 0, nil, &ad); rc != 0 {
			return rtxErr(rc)
		}
		offered = int(C.rtx_accum_samples(acc))
		if ad.open_tiles == 0 {
			break
		}
		if onPass != nil && !onPass(offered, uint64(ad.open_tiles), uint64(ad.open_pixels)) {
			break
		}
	}
	text := make([]byte, int(C.rtx_ppm_max_bytes(cam.image_width, cam.image_height)))
	var n C.uint64_t
	if rc := C.rtx_accum_ppm(acc, (*C.char)(unsafe.Pointer(&text[0])), C.uint64_t(len(text)), &n); rc != 0 {
		return rtxErr(rc)
	}
	if rc := C.rtx_device_check(0); rc != 0 {
		return rtxErr(rc)
	}
	_, err = writer.Write(text[:int(n)])
	return err
}

// Guide is one pixel of the first-hit guide images (rtx_guide, rtx.h "denoised previews"): the mean over a range of
// samples of the albedo, the normal and the depth at the first hit of the render's own camera ray; Cover is the share
// of the samples that hit anything, and Depth is 0 where none did.
type Guide struct {
	Albedo Vec3
	Cover  float32
	Normal Vec3
	Depth  float32
}

// DenoiseParams are the preview filter's (rtx_denoise_params); DefaultDenoiseParams returns rtx_denoise_defaults'.
type DenoiseParams struct {
	Iterations                             uint32
	SigmaNormal, SigmaDepth, SigmaLuminance float32
}

func DefaultDenoiseParams() DenoiseParams {
	var p C.rtx_denoise_params
	C.rtx_denoise_defaults(&p)
	return DenoiseParams{Iterations: uint32(p.iterations), SigmaNormal: float32(p.sigma_normal),
		SigmaDepth: float32(p.sigma_depth), SigmaLuminance: float32(p.sigma_luminance)}
}

func (p DenoiseParams) c() C.rtx_denoise_params {
	return C.rtx_denoise_params{iterations: C.uint32_t(p.Iterations), sigma_normal: C.float(p.SigmaNormal),
		sigma_depth: C.float(p.SigmaDepth), sigma_luminance: C.float(p.SigmaLuminance)}
}

// GuideImages is the first hit of GetRay (camera.go:265-299) for every pixel on the GPU, averaged over samples
// [firstSample, firstSample + count) (rtx_guides): guides[y * W + x] belongs to pixel (x, y).  The world is
// flattened and uploaded for the call, as in HitBatch.
func (c *Camera) GuideImages(world Hittable, seed uint64, firstSample, count uint32) ([]Guide, error) {
	c.init()
	cam := c.gpuCamera()
	region := C.rtx_region{x0: 0, y0: 0, width: cam.image_width, height: cam.image_height, rank: 0, world: 1, stripe: 0}
	n := int(cam.image_width) * int(cam.image_height)
	out := make([]Guide, n)
	if n == 0 {
		return out, nil
	}
	scene, err := sceneOf(world, seed)
	if errors.Is(err, errUnsupported) {
		return nil, errFallback
	}
	if err != nil {
		return nil, err
	}
	defer C.rtx_scene_destroy(scene)
	buf, ptr := alignedBytes(uintptr(n) * unsafe.Sizeof(C.rtx_guide{}))
	var pin runtime.Pinner
	defer pin.Unpin()
	pin.Pin(&buf[0])
	guides := (*C.rtx_guide)(ptr)
	if rc := C.rtx_guides(scene, &cam, C.uint64_t(seed), &region, C.uint32_t(firstSample), C.uint32_t(count), guides, nil); rc != 0 {
		if gpuMissing(rc) {
			return nil, errFallback
		}
		return nil, rtxErr(rc)
	}
	v3 := func(a [3]C.float) Vec3 { return NewVec3(float32(a[0]), float32(a[1]), float32(a[2])) }
	for i, rec := range unsafe.Slice(guides, n) {
		var g C.rtx_guide = rec
		out[i] = Guide{Albedo: v3(g.albedo), Cover: float32(g.cover), Normal: v3(g.normal), Depth: float32(g.depth)}
	}
	return out, nil
}

// Denoise is the preview filter (rtx_denoise) on the GPU: rgb and variance are a resolved width x rows image and the
// variance of its mean, three float32 per pixel; guides are GuideImages' of the same pixels.  It returns the
// filtered image.
func Denoise(rgb, variance []float32, guides []Guide, width, rows int, p DenoiseParams) ([]float32, error) {
	n := width * rows
	if width < 0 || rows < 0 || len(rgb) != 3*n || len(variance) != 3*n || len(guides) != n {
		return nil, errors.New("rtx: Denoise needs three colour and variance values and one guide per pixel")
	}
	out := make([]float32, 3*n)
	if n == 0 {
		return out, nil
	}
	buf, ptr := alignedBytes(uintptr(n) * unsafe.Sizeof(C.rtx_guide{}))
	var pin runtime.Pinner
	defer pin.Unpin()
	pin.Pin(&buf[0])
	pin.Pin(&rgb[0])
	pin.Pin(&variance[0])
	pin.Pin(&out[0])
	cguides := (*C.rtx_guide)(ptr)
	records := unsafe.Slice(cguides, n)
	for i := range records {
		records[i] = C.rtx_guide{albedo: vec(guides[i].Albedo), cover: C.float(guides[i].Cover),
			normal: vec(guides[i].Normal), depth: C.float(guides[i].Depth)}
	}
	prm := p.c()
	if rc := C.rtx_denoise((*C.float)(unsafe.Pointer(&rgb[0])), (*C.float)(unsafe.Pointer(&variance[0])), cguides, C.uint32_t(width), C.uint32_t(rows), &prm, (*C.float)(unsafe.Pointer(&out[0]))); rc != 0 {
		if gpuMissing(rc) {
			return nil, errFallback
		}
		return nil, rtxErr(rc)
	}
	return out, nil
}

// RenderPreviews is RenderProgressive with a denoised preview after every pass (rtx_accum_preview_ppm): onPreview is
// handed the samples done and the P3 bytes of the filtered image so far, steered by guides over the first
// min(done, guideSamples) samples, and returning false stops the render there.  The bytes written to writer at the
// end are the undenoised image's, exactly RenderProgressive's: a preview is a separate output and changes no render.
func (c *Camera) RenderPreviews(world Hittable, writer io.Writer, passSamples, guideSamples int, p DenoiseParams, onPreview func(done int, ppm []byte) bool) error {
	c.init()
	cfg := c.gpuConfig()
	if passSamples <= 0 {
		passSamples = c.samplesPerPixel
	}
	scene, err := sceneOf(world, cfg.seed)
	if err != nil {
		return err
	}
	defer C.rtx_scene_destroy(scene) // (deferred calls run last in, first out: the accumulator goes first)
	cam := c.gpuCamera()
	region := C.rtx_region{x0: 0, y0: 0, width: cam.image_width, height: cam.image_height, rank: 0, world: 1, stripe: 0}
	var acc *C.rtx_accum
	if rc := C.rtx_accum_create(scene, &cam, C.uint64_t(cfg.seed), &region, &acc); rc != 0 {
		return rtxErr(rc)
	}
	defer C.rtx_accum_destroy(acc)
	prm := p.c()
	text := make([]byte, int(C.rtx_ppm_max_bytes(cam.image_width, cam.image_height)))
	var n C.uint64_t
	for done := 0; done < c.samplesPerPixel; {
		count := min(passSamples, c.samplesPerPixel-done)
		if rc := C.rtx_accum_add(acc, C.uint32_t(count), nil, 0, nil); rc != 0 {
			return rtxErr(rc)
		}
		done = int(C.rtx_accum_samples(acc))
		if onPreview == nil {
			continue
		}
		if rc := C.rtx_accum_preview_ppm(acc, C.uint32_t(guideSamples), &prm, (*C.char)(unsafe.Pointer(&text[0])), C.uint64_t(len(text)), &n); rc != 0 {
			return rtxErr(rc)
		}
		if !onPreview(done, text[:int(n)]) {
			break
		}
	}
	if rc := C.rtx_accum_ppm(acc, (*C.char)(unsafe.Pointer(&text[0])), C.uint64_t(len(text)), &n); rc != 0 {
		return rtxErr(rc)
	}
	if rc := C.rtx_device_check(0); rc != 0 { // the passes ran without stats: the sticky error word, once
		return rtxErr(rc)
	}
	_, err = writer.Write(text[:int(n)])
	return err
}

// renderOnDevices renders on `gpus` devices and writes Render's P3 bytes; errFallback when the GPU
// path cannot carry the render (nothing has been written then).
func (c *Camera) renderOnDevices(world Hittable, writer io.Writer, seed uint64, gpus int) error {
	c.init() // Camera.init (idempotent, sync.Once): the derived state below (camera.go:128-165)
	scene, err := sceneOf(world, seed)
	var re *rtxError
	if errors.Is(err, errUnsupported) || (errors.As(err, &re) && gpuMissing(re.code)) {
		return errFallback
	}
	if err != nil {
		return err
	}
	// Destroying the last scene on a device also frees the library's sample scratch there, so
	// nothing stays pinned in HBM after Render returns.
	defer C.rtx_scene_destroy(scene)

	w, h := int(c.imageWidth), int(c.imageHeight)
	cam := c.gpuCamera()
	// Render + the P3 text (header included) on the device: rtx_render_ppm on the current device for one
	// GPU; for several, rtx_render_ppm_ex (ABI 9) gathers the row-interleaved bands to device 0 over RCCL
	// and encodes them there, so no per-pixel formatting runs on the host at any device count
	// (camera.go:183-188, 212-215 and vec3.go:141-166 on the GPU, byte-identical).
	text := make([]byte, int(C.rtx_ppm_max_bytes(C.uint32_t(w), C.uint32_t(h))))
	var n C.uint64_t
	var rc C.int
	if gpus <= 1 {
		rc = C.rtx_render_ppm(scene, &cam, C.uint64_t(seed), (*C.char)(unsafe.Pointer(&text[0])),
			C.uint64_t(len(text)), &n, nil)
	} else {
		rc = C.rtx_render_ppm_ex(scene, &cam, C.uint64_t(seed), C.int(gpus), (*C.char)(unsafe.Pointer(&text[0])),
			C.uint64_t(len(text)), &n, nil)
	}
	if rc != 0 {
		if gpuMissing(rc) {
			return errFallback
		}
		return rtxErr(rc)
	}
	_, err = writer.Write(text[:int(n)])
	return err
}
