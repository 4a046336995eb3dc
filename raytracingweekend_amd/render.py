"""Host-side Python API over the C ABI: the render loop of
RayTracingWeekend.cpp:195-289 (scene -> canvas -> PPM) with the per-pixel work
on the GPU.

    from raytracingweekend_amd import render
    canvas, stats = render.render("cornell_box", 400, 400, spp=64, max_depth=100)
    render.write_ppm("x64/1.ppm", canvas, 400, 400)

Multi-GPU (one process per GPU, torch.distributed over RCCL): see
raytracingweekend_amd.distributed.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import numpy as np

from . import _abi
from ._abi import check, lib


# rtw_query_hit (include/rtw_query.h) as a numpy record: 64 bytes
QUERY_HIT_DTYPE = np.dtype([("t", np.float64), ("p", np.float64, 3), ("n", np.float64, 3), ("prim", np.int32),
                            ("material", np.int32)])


class SceneDesc:
    """A reference scene built with the host C++ scene API and flattened
    (rtw_scene_builtin).  Owns the library-allocated rtw_scene_desc."""

    def __init__(self, name: str, aspect: float, use_bvh: bool = False):
        self.name = name
        self.aspect = float(aspect)
        self.use_bvh = bool(use_bvh)
        p = C.POINTER(_abi.rtw_scene_desc)()
        check(lib().rtw_scene_builtin(name.encode(), self.aspect, int(use_bvh), C.byref(p)), "rtw_scene_builtin")
        self.ptr = p

    @property
    def desc(self) -> _abi.rtw_scene_desc:
        """A ctypes view of the library-owned descriptor.  The view keeps this
        SceneDesc (its owner) alive, so `SceneDesc(...).desc` of a temporary
        stays valid as long as the view does (the reference holds its scene
        graph by shared_ptr, Scene/scene.h:18-40)."""
        if not self.ptr:
            raise ValueError("SceneDesc is closed")
        view = self.ptr.contents
        view._rtw_owner = self
        return view

    @property
    def camera(self) -> _abi.rtw_camera_desc:
        """A view of the descriptor's camera; through its base view it keeps
        this SceneDesc alive (see `desc`)."""
        return self.desc.camera

    def close(self):
        if self.ptr:
            lib().rtw_scene_desc_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeviceScene:
    """A scene uploaded to one GPU (rtw_scene_upload)."""

    def __init__(self, scene: SceneDesc, device: int = 0):
        self.scene = scene
        self.device = device
        h = C.c_void_p()
        check(lib().rtw_scene_upload(device, scene.ptr, C.byref(h)), "rtw_scene_upload")
        self.handle = h

    def render_accumulate(self, nx: int, ny: int, spp: int, max_depth: int, seed: int = 0, *,
                          spp_begin: int = 0, spp_count: int = 0, row_begin: int = 0, row_step: int = 1,
                          accum=None, camera: Optional[_abi.rtw_camera_desc] = None,
                          collect_kernel_times: bool = False, wavefront_paths: int = 0, precision: str = "fp64"):
        """Add the per-pixel radiance sums of the selected samples into `accum`
        (a float64 numpy array of nx*ny*3, or a torch float64 CUDA tensor on
        this device).  precision "fp64" is the reference's arithmetic (parity
        mode); "fp32" the fast mode (statistical parity only).  Returns
        (accum, stats dict)."""
        if accum is None:
            accum = np.zeros(nx * ny * 3, dtype=np.float64)
        ptr, on_device = self._accum_ptr(accum, nx, ny, "accum")
        prm = _abi.rtw_render_params(nx=nx, ny=ny, spp=spp, max_depth=max_depth, seed=seed, spp_begin=spp_begin,
                                     spp_count=spp_count, row_begin=row_begin, row_step=row_step,
                                     accum_on_device=on_device, collect_kernel_times=int(collect_kernel_times),
                                     wavefront_paths=wavefront_paths, precision=_precision(precision))
        st = _abi.rtw_stats()
        cam = camera if camera is not None else self.scene.camera
        check(lib().rtw_render_accumulate(self.handle, C.byref(cam), C.byref(prm), ptr, C.byref(st)),
              "rtw_render_accumulate")
        return accum, st.as_dict()

    def _accum_ptr(self, accum, nx: int, ny: int, name: str):
        """(pointer, accum_on_device) of an accumulator: a float64 numpy array
        of nx*ny*3, or a torch float64 tensor on this device (synchronized)."""
        if isinstance(accum, np.ndarray):
            if accum.dtype != np.float64 or accum.size != nx * ny * 3 or not accum.flags["C_CONTIGUOUS"]:
                raise ValueError(f"{name} must be a contiguous float64 array of nx*ny*3")
            return accum.ctypes.data_as(C.c_void_p), 0
        import torch
        if accum.dtype != torch.float64 or accum.numel() != nx * ny * 3 or not accum.is_contiguous():
            raise ValueError(f"{name} must be a contiguous float64 tensor of nx*ny*3")
        if not accum.is_cuda or accum.device.index != self.device:
            raise ValueError(f"a torch {name} must live on this scene's GPU (cuda:{self.device})")
        torch.cuda.synchronize(accum.device)
        return C.c_void_p(accum.data_ptr()), 1

    def render_moments(self, nx: int, ny: int, spp: int, max_depth: int, seed: int = 0, *,
                       spp_begin: int = 0, spp_count: int = 0, row_begin: int = 0, row_step: int = 1,
                       accum=None, accum_sq=None, camera: Optional[_abi.rtw_camera_desc] = None,
                       collect_kernel_times: bool = False, wavefront_paths: int = 0, precision: str = "fp64"):
        """render_accumulate, and additionally the per-pixel sums of the
        squares of the same samples into `accum_sq` (rtw_render_accumulate_moments:
        the raw second moments rtw_noise.h's estimate needs).  Both buffers
        are float64 numpy arrays of nx*ny*3, or both torch float64 CUDA
        tensors on this device; one given alone gets a zero partner of its
        kind.  Returns (accum, accum_sq, stats dict)."""
        if accum is None and accum_sq is None:
            accum = np.zeros(nx * ny * 3, dtype=np.float64)
        if accum is None:
            accum = _zeros_like(accum_sq)
        if accum_sq is None:
            accum_sq = _zeros_like(accum)
        ptr, ptr_sq, on_device = self._moment_buffers(accum, accum_sq, nx, ny)
        prm = _abi.rtw_render_params(nx=nx, ny=ny, spp=spp, max_depth=max_depth, seed=seed, spp_begin=spp_begin,
                                     spp_count=spp_count, row_begin=row_begin, row_step=row_step,
                                     accum_on_device=on_device, collect_kernel_times=int(collect_kernel_times),
                                     wavefront_paths=wavefront_paths, precision=_precision(precision))
        st = _abi.rtw_stats()
        cam = camera if camera is not None else self.scene.camera
        check(lib().rtw_render_accumulate_moments(self.handle, C.byref(cam), C.byref(prm), ptr, ptr_sq,
                                                  C.byref(st)), "rtw_render_accumulate_moments")
        return accum, accum_sq, st.as_dict()

    def _moment_buffers(self, accum, accum_sq, nx: int, ny: int):
        """(pointer, pointer, accum_on_device) of a pair of moment buffers:
        both numpy, or both torch on this device (a mix: ValueError)."""
        if isinstance(accum, np.ndarray) != isinstance(accum_sq, np.ndarray):
            raise ValueError("accum and accum_sq must both be numpy arrays or both be torch tensors on this device")
        ptr, on_device = self._accum_ptr(accum, nx, ny, "accum")
        ptr_sq, _ = self._accum_ptr(accum_sq, nx, ny, "accum_sq")
        return ptr, ptr_sq, on_device

    def noise_estimate(self, accum, accum_sq, nx: int, ny: int, n: int, floor: float = 1e-2,
                       want_stderr: bool = True):
        """The standard-error map and summary of `n` samples' raw moments
        (rtw_noise.h).  Torch tensors on this device go through the device
        estimator (rtw_noise_estimate_device; the map is a tensor); numpy
        arrays fall through to the host function, render.noise_estimate.
        Returns (stderr or None, summary dict)."""
        return self._noise_estimate(accum, accum_sq, nx, ny, floor, want_stderr, n=n)

    def _noise_estimate(self, accum, accum_sq, nx: int, ny: int, floor: float, want_stderr: bool, n=None, counts=None):
        """noise_estimate (n) and noise_estimate_counts (counts): numpy arrays
        go to the host functions, tensors to the device entry points."""
        if isinstance(accum, np.ndarray) and isinstance(accum_sq, np.ndarray):
            return _noise_estimate(accum, accum_sq, nx, ny, floor, want_stderr, n, counts)
        ptr, ptr_sq, _ = self._moment_buffers(accum, accum_sq, nx, ny)
        import torch
        se = torch.empty_like(accum) if want_stderr else None
        out = _abi.rtw_noise_summary()
        tail = (floor, C.c_void_p(se.data_ptr()) if want_stderr else None, C.byref(out))
        if counts is None:
            check(lib().rtw_noise_estimate_device(self.handle, ptr, ptr_sq, nx, ny, n, *tail),
                  "rtw_noise_estimate_device")
        else:
            check(lib().rtw_noise_estimate_counts_device(self.handle, ptr, ptr_sq,
                                                         self._u32_ptr(counts, nx * ny, "counts", True), nx, ny, *tail),
                  "rtw_noise_estimate_counts_device")
        return se, out.as_dict()

    # ---- adaptive sampling (include/rtw_adaptive.h) ---------------------------
    def _u32_ptr(self, a, n: int, name: str, want_device: bool):
        """Pointer of a uint32 buffer of `n` entries of the same kind as the
        moments: numpy, or a torch tensor on this device (int32 is accepted:
        torch has no unsigned 32-bit arithmetic; the values are below 2^31)."""
        if isinstance(a, np.ndarray):
            if want_device:
                raise ValueError(f"{name} must be a torch tensor on this device, like the moments")
            if a.dtype != np.uint32 or a.size != n or not a.flags["C_CONTIGUOUS"]:
                raise ValueError(f"{name} must be a contiguous uint32 array of {n} entries")
            return a.ctypes.data_as(C.c_void_p)
        import torch
        if not want_device:
            raise ValueError(f"{name} must be a numpy array, like the moments")
        if a.dtype not in (torch.int32, getattr(torch, "uint32", torch.int32)) or a.numel() != n \
                or not a.is_contiguous():
            raise ValueError(f"{name} must be a contiguous int32 tensor of {n} entries")
        if not a.is_cuda or a.device.index != self.device:
            raise ValueError(f"a torch {name} must live on this scene's GPU (cuda:{self.device})")
        torch.cuda.synchronize(a.device)
        return C.c_void_p(a.data_ptr())

    def render_active(self, nx: int, ny: int, spp: int, max_depth: int, seed: int = 0, *, active, accum, accum_sq=None,
                      counts=None, spp_begin: int = 0, spp_count: int = 0, row_begin: int = 0, row_step: int = 1,
                      camera: Optional[_abi.rtw_camera_desc] = None, collect_kernel_times: bool = False,
                      wavefront_paths: int = 0, precision: str = "fp64"):
        """rtw_render_accumulate_active: the samples [spp_begin, spp_begin +
        spp_count) of the pixels listed in `active` (indices j*nx + i,
        strictly ascending), added to those pixels of `accum`, `accum_sq`
        (optional) and, as a sample count, `counts` (optional).  All buffers
        are numpy arrays (uint32 list and counts) or all torch tensors on this
        device (int32 list and counts).  Returns the stats dict."""
        on_device = not isinstance(accum, np.ndarray)
        ptr, _ = self._accum_ptr(accum, nx, ny, "accum")
        ptr_sq = None
        if accum_sq is not None:
            _, ptr_sq, _ = self._moment_buffers(accum, accum_sq, nx, ny)
        n_active = int(active.size if isinstance(active, np.ndarray) else active.numel())
        ptr_list = self._u32_ptr(active, n_active, "active", on_device)
        ptr_counts = self._u32_ptr(counts, nx * ny, "counts", on_device) if counts is not None else None
        prm = _abi.rtw_render_params(nx=nx, ny=ny, spp=spp, max_depth=max_depth, seed=seed, spp_begin=spp_begin,
                                     spp_count=spp_count, row_begin=row_begin, row_step=row_step,
                                     accum_on_device=int(on_device), collect_kernel_times=int(collect_kernel_times),
                                     wavefront_paths=wavefront_paths, precision=_precision(precision))
        st = _abi.rtw_stats()
        cam = camera if camera is not None else self.scene.camera
        check(lib().rtw_render_accumulate_active(self.handle, C.byref(cam), C.byref(prm), ptr_list, n_active, ptr,
                                                 ptr_sq, ptr_counts, C.byref(st)), "rtw_render_accumulate_active")
        return st.as_dict()

    def select_active(self, accum, accum_sq, counts, nx: int, ny: int, *, target_rel: float, max_count: int,
                      floor: float = 1e-2):
        """The ascending list of the active pixels (rtw_adaptive.h): torch
        tensors on this device go through rtw_adaptive_select_device and give
        an int32 tensor, numpy arrays through the host function,
        render.select_active."""
        if isinstance(accum, np.ndarray):
            return select_active(accum, accum_sq, counts, nx, ny, target_rel=target_rel, max_count=max_count,
                                 floor=floor)
        import torch
        ptr, ptr_sq, _ = self._moment_buffers(accum, accum_sq, nx, ny)
        ptr_counts = self._u32_ptr(counts, nx * ny, "counts", True)
        out = torch.empty(nx * ny, dtype=torch.int32, device=accum.device)
        torch.cuda.synchronize(accum.device)
        n = C.c_uint64()
        check(lib().rtw_adaptive_select_device(self.handle, ptr, ptr_sq, ptr_counts, nx, ny, floor, target_rel,
                                               max_count, C.c_void_p(out.data_ptr()), C.byref(n)),
              "rtw_adaptive_select_device")
        return out[:n.value]

    def select_active_window(self, accum, accum_sq, counts, nx: int, ny: int, *, target_rel: float, max_count: int,
                             radius: int, min_count: int = 0, floor: float = 1e-2):
        """The ascending list of the window-active pixels
        (rtw_adaptive_window.h): torch tensors on this device go through
        rtw_adaptive_select_window_device and give an int32 tensor, numpy
        arrays through the host function, render.select_active_window."""
        if isinstance(accum, np.ndarray):
            return select_active_window(accum, accum_sq, counts, nx, ny, target_rel=target_rel, max_count=max_count,
                                        radius=radius, min_count=min_count, floor=floor)
        import torch
        ptr, ptr_sq, _ = self._moment_buffers(accum, accum_sq, nx, ny)
        ptr_counts = self._u32_ptr(counts, nx * ny, "counts", True)
        out = torch.empty(nx * ny, dtype=torch.int32, device=accum.device)
        torch.cuda.synchronize(accum.device)
        n = C.c_uint64()
        check(lib().rtw_adaptive_select_window_device(self.handle, ptr, ptr_sq, ptr_counts, nx, ny, floor, target_rel,
                                                      min_count, max_count, radius, C.c_void_p(out.data_ptr()),
                                                      C.byref(n)), "rtw_adaptive_select_window_device")
        return out[:n.value]

    def noise_estimate_counts(self, accum, accum_sq, counts, nx: int, ny: int, floor: float = 1e-2,
                              want_stderr: bool = True):
        """noise_estimate with a per-pixel sample count (rtw_noise_estimate_counts
        [_device]).  Returns (stderr or None, summary dict)."""
        return self._noise_estimate(accum, accum_sq, nx, ny, floor, want_stderr, counts=counts)

    def finalize_counts(self, accum, counts, nx: int, ny: int):
        """canvas = min(sqrt(accum / counts[p]), 1) (rtw_finalize_canvas_counts
        [_device]): a tensor for tensors, an array for arrays."""
        return self._finalize(accum, nx, ny, "accum", counts=counts)

    def _finalize(self, sums, nx: int, ny: int, name: str, n=None, counts=None, canvas=None):
        """The canvas of channel sums over `n` samples, over counts[p], or of
        a mean (neither): numpy arrays go to the host functions, tensors to
        the device entry points (into `canvas`, if given)."""
        if isinstance(sums, np.ndarray):
            return _finalize(sums, nx, ny, n, counts)
        import torch
        ptr, _ = self._accum_ptr(sums, nx, ny, name)
        ptr_counts = self._u32_ptr(counts, nx * ny, "counts", True) if counts is not None else None
        if canvas is None:
            canvas = torch.empty_like(sums)
        torch.cuda.synchronize(sums.device)
        out = C.c_void_p(canvas.data_ptr())
        if counts is not None:
            check(lib().rtw_finalize_canvas_counts_device(self.handle, ptr, ptr_counts, nx, ny, out),
                  "rtw_finalize_canvas_counts_device")
        elif n is not None:
            check(lib().rtw_finalize_canvas_device(self.handle, ptr, nx, ny, n, out), "rtw_finalize_canvas_device")
        else:
            check(lib().rtw_finalize_canvas_mean_device(self.handle, ptr, nx, ny, out),
                  "rtw_finalize_canvas_mean_device")
        return canvas

    def query_active(self, precision: str = "fp64") -> str:
        """rtw_scene_query_active: the traversal kernel an active render of
        this scene launches now."""
        name = C.create_string_buffer(128)
        check(lib().rtw_scene_query_active(self.handle, _precision(precision), name), "rtw_scene_query_active")
        return name.value.decode()

    # ---- the denoiser (include/rtw_denoise.h) ---------------------------------
    def _features_ptr(self, features, nx: int, ny: int):
        """(pointer, on_device) of a feature buffer: float64 of nx*ny*8."""
        n = nx * ny * _abi.RTW_FEATURE_CHANNELS
        if isinstance(features, np.ndarray):
            if features.dtype != np.float64 or features.size != n or not features.flags["C_CONTIGUOUS"]:
                raise ValueError("features must be a contiguous float64 array of nx*ny*8")
            return features.ctypes.data_as(C.c_void_p), 0
        import torch
        if features.dtype != torch.float64 or features.numel() != n or not features.is_contiguous():
            raise ValueError("features must be a contiguous float64 tensor of nx*ny*8")
        if not features.is_cuda or features.device.index != self.device:
            raise ValueError(f"a torch feature buffer must live on this scene's GPU (cuda:{self.device})")
        torch.cuda.synchronize(features.device)
        return C.c_void_p(features.data_ptr()), 1

    def render_features(self, nx: int, ny: int, spp: int, seed: int = 0, *, spp_begin: int = 0, spp_count: int = 0,
                        row_begin: int = 0, row_step: int = 1, features=None,
                        camera: Optional[_abi.rtw_camera_desc] = None):
        """rtw_render_features: ADD the first-hit feature sums (albedo, normal,
        1/t, coverage: eight per pixel) of the selected samples, the camera
        rays render_accumulate traces with the same arguments, into `features`
        (a float64 numpy array of nx*ny*8, or a torch float64 tensor on this
        device).  Returns (features, stats dict)."""
        if features is None:
            features = np.zeros(nx * ny * _abi.RTW_FEATURE_CHANNELS, dtype=np.float64)
        ptr, on_device = self._features_ptr(features, nx, ny)
        prm = _abi.rtw_render_params(nx=nx, ny=ny, spp=spp, max_depth=1, seed=seed, spp_begin=spp_begin,
                                     spp_count=spp_count, row_begin=row_begin, row_step=row_step,
                                     accum_on_device=on_device, precision=_abi.PRECISIONS["fp64"])
        st = _abi.rtw_stats()
        cam = camera if camera is not None else self.scene.camera
        check(lib().rtw_render_features(self.handle, C.byref(cam), C.byref(prm), ptr, C.byref(st)),
              "rtw_render_features")
        return features, st.as_dict()

    def query_features(self) -> str:
        """rtw_scene_query_features: the kernel render_features launches."""
        name = C.create_string_buffer(128)
        check(lib().rtw_scene_query_features(self.handle, name), "rtw_scene_query_features")
        return name.value.decode()

    def denoise(self, accum, accum_sq, features, nx: int, ny: int, *, n: int = 0, counts=None, feature_spp: int,
                want_variance: bool = False, **params):
        """The a-trous filter (rtw_denoise.h) of raw moments with `n` samples
        per pixel or a per-pixel `counts`.  Torch tensors on this device go
        through rtw_denoise_device and give tensors; numpy arrays fall through
        to the host function, render.denoise (the same bits).  `params`:
        iterations, sigma_l, sigma_z, eps_a, normal_power_log2.  Returns the
        denoised linear mean, or (mean, variance) with want_variance."""
        if isinstance(accum, np.ndarray):
            return denoise(accum, accum_sq, features, nx, ny, n=n, counts=counts, feature_spp=feature_spp,
                           want_variance=want_variance, **params)
        import torch
        ptr, ptr_sq, _ = self._moment_buffers(accum, accum_sq, nx, ny)
        ptr_f, on_device = self._features_ptr(features, nx, ny)
        if not on_device:
            raise ValueError("features must be a torch tensor on this device, like the moments")
        ptr_counts = self._u32_ptr(counts, nx * ny, "counts", True) if counts is not None else None
        out = torch.empty_like(accum)
        var = torch.empty_like(accum) if want_variance else None
        torch.cuda.synchronize(accum.device)
        prm = denoise_params(**params)
        check(lib().rtw_denoise_device(self.handle, ptr, ptr_sq, ptr_counts, n, ptr_f, feature_spp, nx, ny,
                                       C.byref(prm), C.c_void_p(out.data_ptr()),
                                       C.c_void_p(var.data_ptr()) if want_variance else None), "rtw_denoise_device")
        return (out, var) if want_variance else out

    def finalize_mean(self, mean, nx: int, ny: int):
        """canvas = min(sqrt(mean), 1) of a denoised mean
        (rtw_finalize_canvas_mean[_device])."""
        return self._finalize(mean, nx, ny, "mean")

    # ---- ray queries (include/rtw_query.h) ------------------------------------
    def _rng_ptr(self, rng, n: int, want_device: bool):
        """Pointer of n minstd states: a uint32 numpy array, or a torch int32 /
        uint32 tensor on this device (the same kind as the rays)."""
        if rng is None:
            return None
        if isinstance(rng, np.ndarray):
            if want_device or rng.dtype != np.uint32 or rng.size != n or not rng.flags["C_CONTIGUOUS"]:
                raise ValueError("rng must be a contiguous uint32 array of n states, of the rays' kind")
            return rng.ctypes.data_as(C.c_void_p)
        import torch
        kinds = [torch.int32] + ([torch.uint32] if hasattr(torch, "uint32") else [])
        if (not want_device or rng.dtype not in kinds or rng.numel() != n or not rng.is_contiguous() or not rng.is_cuda
                or rng.device.index != self.device):
            raise ValueError("rng must be a contiguous int32 / uint32 tensor of n states on this scene's GPU")
        return C.c_void_p(rng.data_ptr())

    def trace_rays(self, rays, rng=None, *, occluded: bool = False):
        """rtw_trace_closest / rtw_trace_occluded of the caller's rays: an
        (n, 8) float64 numpy array or CUDA tensor of this device with rows
        (o, d, time, t_max).  `rng` (n minstd states, updated in place) is
        needed for a scene with media only.  Results come back in the rays'
        kind.  Closest: a structured array with fields t, p, n, prim, material
        (rtw_query_hit), or for tensors a dict of views t, p, n, prim,
        material over one (n, 8) float64 buffer, also under "records".
        occluded=True: n uint8 flags.  Tensors are passed by data_ptr(),
        nothing is copied through the host.  The call's stats are left in
        self.last_query_stats."""
        on_device = not isinstance(rays, np.ndarray)
        if on_device:
            import torch
            if (rays.dtype != torch.float64 or rays.dim() != 2 or rays.shape[1] != 8 or not rays.is_contiguous()
                    or not rays.is_cuda or rays.device.index != self.device):
                raise ValueError("rays must be a contiguous (n, 8) float64 tensor on this scene's GPU")
            n = rays.shape[0]
            out = (torch.empty(n, dtype=torch.uint8, device=rays.device) if occluded
                   else torch.empty((n, 8), dtype=torch.float64, device=rays.device))
            torch.cuda.synchronize(rays.device)
            p_rays, p_out = C.c_void_p(rays.data_ptr()), C.c_void_p(out.data_ptr())
        else:
            if rays.dtype != np.float64 or rays.ndim != 2 or rays.shape[1] != 8 or not rays.flags["C_CONTIGUOUS"]:
                raise ValueError("rays must be a contiguous (n, 8) float64 array")
            n = rays.shape[0]
            out = np.empty(n, dtype=np.uint8) if occluded else np.empty(n, dtype=QUERY_HIT_DTYPE)
            p_rays, p_out = rays.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
        prm = _abi.rtw_query_params(on_device=int(on_device), precision=_abi.RTW_PRECISION_FP64)
        st = _abi.rtw_stats()
        fn = lib().rtw_trace_occluded if occluded else lib().rtw_trace_closest
        check(fn(self.handle, p_rays, n, self._rng_ptr(rng, n, on_device), C.byref(prm), p_out, C.byref(st)),
              "rtw_trace_occluded" if occluded else "rtw_trace_closest")
        self.last_query_stats = st.as_dict()
        if occluded or not on_device:
            return out
        import torch
        ids = out[:, 7:8].view(torch.int32)
        return {"records": out, "t": out[:, 0], "p": out[:, 1:4], "n": out[:, 4:7], "prim": ids[:, 0],
                "material": ids[:, 1]}

    def camera_rays(self, nx: int, ny: int, spp: int, seed: int = 0, *, spp_begin: int = 0, spp_count: int = 0,
                    row_begin: int = 0, row_step: int = 1, device: bool = False,
                    camera: Optional[_abi.rtw_camera_desc] = None):
        """rtw_camera_rays: the first rays render_accumulate traces with the
        same arguments, as (rays (n, 8) float64, rng n states after the
        camera's draws), at the render's pass-local sample ids q = (s -
        spp_begin) * npix + row * nx + i.  device=True: CUDA tensors (rng
        int32) of this device, else numpy arrays (rng uint32)."""
        step = row_step if row_step > 0 else 1
        rows = max(0, (ny - row_begin + step - 1) // step)
        count = spp_count if spp_count else spp - spp_begin
        n = max(0, count) * rows * nx
        if device:
            import torch
            dev = torch.device("cuda", self.device)
            rays = torch.empty((n, 8), dtype=torch.float64, device=dev)
            rng = torch.empty(n, dtype=torch.int32, device=dev)
            torch.cuda.synchronize(dev)
            p_rays, p_rng = C.c_void_p(rays.data_ptr()), C.c_void_p(rng.data_ptr())
        else:
            rays, rng = np.empty((n, 8), dtype=np.float64), np.empty(n, dtype=np.uint32)
            p_rays, p_rng = rays.ctypes.data_as(C.c_void_p), rng.ctypes.data_as(C.c_void_p)
        prm = _abi.rtw_render_params(nx=nx, ny=ny, spp=spp, max_depth=1, seed=seed, spp_begin=spp_begin,
                                     spp_count=spp_count, row_begin=row_begin, row_step=row_step,
                                     accum_on_device=int(device), precision=_abi.PRECISIONS["fp64"])
        cam = camera if camera is not None else self.scene.camera
        if n == 0:
            return rays, rng
        check(lib().rtw_camera_rays(self.handle, C.byref(cam), C.byref(prm), p_rays, p_rng, n), "rtw_camera_rays")
        return rays, rng

    def query_trace(self) -> Tuple[str, str]:
        """rtw_scene_query_trace: the kernels trace_rays launches, (closest,
        occluded)."""
        a, b = C.create_string_buffer(128), C.create_string_buffer(128)
        check(lib().rtw_scene_query_trace(self.handle, a, b), "rtw_scene_query_trace")
        return a.value.decode(), b.value.decode()

    # ---- radiance queries (include/rtw_radiance.h) ------------------------------
    def trace_radiance(self, rays, spp: int, max_depth: int, *, seed: int = 0, spp_begin: int = 0,
                       first_key: int = 0, rng=None, out=None, wavefront_paths: int = 0,
                       precision: str = "fp64"):
        """rtw_trace_radiance of the caller's rays ((n, 8) float64 rows (o, d,
        time, t_max), numpy or a CUDA tensor of this device as trace_rays
        takes them): path-traces samples [spp_begin, spp_begin + spp) of every
        ray, ray k keyed first_key + k, and ADDS each ray's sum to row k of
        `out` ((n, 3) float64 of the rays' kind; None: fresh zeros).  `rng`
        (n minstd states of the rays' kind, read only): ray k's one sample
        starts from rng[k] instead (spp must be 1) -- with camera_rays' output
        these are a render's own paths.  Returns the sums; the call's stats are
        left in self.last_query_stats."""
        on_device = not isinstance(rays, np.ndarray)
        if on_device:
            import torch
            if (rays.dtype != torch.float64 or rays.dim() != 2 or rays.shape[1] != 8 or not rays.is_contiguous()
                    or not rays.is_cuda or rays.device.index != self.device):
                raise ValueError("rays must be a contiguous (n, 8) float64 tensor on this scene's GPU")
            n = rays.shape[0]
            if out is None:
                out = torch.zeros((n, 3), dtype=torch.float64, device=rays.device)
            elif (isinstance(out, np.ndarray) or out.dtype != torch.float64 or tuple(out.shape) != (n, 3)
                  or not out.is_contiguous() or not out.is_cuda or out.device.index != self.device):
                raise ValueError("out must be a contiguous (n, 3) float64 tensor on this scene's GPU")
            torch.cuda.synchronize(rays.device)
            p_rays, p_out = C.c_void_p(rays.data_ptr()), C.c_void_p(out.data_ptr())
        else:
            if rays.dtype != np.float64 or rays.ndim != 2 or rays.shape[1] != 8 or not rays.flags["C_CONTIGUOUS"]:
                raise ValueError("rays must be a contiguous (n, 8) float64 array")
            n = rays.shape[0]
            if out is None:
                out = np.zeros((n, 3), dtype=np.float64)
            elif (not isinstance(out, np.ndarray) or out.dtype != np.float64 or out.shape != (n, 3)
                  or not out.flags["C_CONTIGUOUS"]):
                raise ValueError("out must be a contiguous (n, 3) float64 array")
            p_rays, p_out = rays.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
        prm = _abi.rtw_radiance_params(max_depth=max_depth, spp_begin=spp_begin, spp_count=spp,
                                       on_device=int(on_device), seed=seed, first_key=first_key,
                                       precision=_abi.PRECISIONS[precision], wavefront_paths=wavefront_paths)
        st = _abi.rtw_stats()
        check(lib().rtw_trace_radiance(self.handle, p_rays, n, self._rng_ptr(rng, n, on_device), C.byref(prm), p_out,
                                       C.byref(st)), "rtw_trace_radiance")
        self.last_query_stats = st.as_dict()
        return out

    def query_radiance(self) -> str:
        """rtw_scene_query_radiance: the kernel(s) trace_radiance launches under
        the current environment."""
        a = C.create_string_buffer(128)
        check(lib().rtw_scene_query_radiance(self.handle, a), "rtw_scene_query_radiance")
        return a.value.decode()

    def finalize_device(self, accum, nx: int, ny: int, spp: int, canvas=None):
        """canvas = min(sqrt(accum / spp), 1) on the GPU (torch float64 CUDA
        tensors of nx*ny*3 on this device).  Returns the canvas tensor."""
        if isinstance(accum, np.ndarray) or not accum.is_cuda:
            raise ValueError("accum must be a contiguous float64 CUDA tensor of nx*ny*3")
        return self._finalize(accum, nx, ny, "accum", n=spp, canvas=canvas)

    def query(self) -> dict:
        """rtw_scene_query: run layout, feature bits, the traversal kernel a
        render launches now and the device code's build id."""
        info = _abi.rtw_scene_info()
        check(lib().rtw_scene_query(self.handle, C.byref(info)), "rtw_scene_query")
        return info.as_dict()

    def quantize_device(self, canvas, nx: int, ny: int, out=None):
        """PPM channel values int(255.99f * c) of a device canvas, on the GPU
        (rtw_quantize_canvas_device).  Returns an int32 CUDA tensor."""
        import torch
        if not (canvas.is_cuda and canvas.dtype == torch.float64 and canvas.numel() == nx * ny * 3
                and canvas.is_contiguous()):
            raise ValueError("canvas must be a contiguous float64 CUDA tensor of nx*ny*3")
        if out is None:
            out = torch.empty(nx * ny * 3, dtype=torch.int32, device=canvas.device)
        torch.cuda.synchronize(canvas.device)
        check(lib().rtw_quantize_canvas_device(self.handle, C.c_void_p(canvas.data_ptr()), nx, ny,
                                               C.c_void_p(out.data_ptr())), "rtw_quantize_canvas_device")
        return out

    def close(self):
        if self.handle:
            lib().rtw_scene_free(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def render_multi(scenes, nx: int, ny: int, spp: int, max_depth: int, seed: int = 0, *, spp_begin: int = 0,
                 spp_count: int = 0, row_begin: int = 0, row_step: int = 1, accum=None,
                 camera: Optional[_abi.rtw_camera_desc] = None, collect_kernel_times: bool = False,
                 precision: str = "fp64"):
    """rtw_render_multi over DeviceScenes on distinct GPUs (one process, one
    host thread per GPU, RCCL reduce to scenes[0]'s device).  `accum`: float64
    numpy array, or torch float64 tensor on scenes[0]'s device."""
    if accum is None:
        accum = np.zeros(nx * ny * 3, dtype=np.float64)
    on_device = 0
    if isinstance(accum, np.ndarray):
        if accum.dtype != np.float64 or accum.size != nx * ny * 3 or not accum.flags["C_CONTIGUOUS"]:
            raise ValueError("accum must be a contiguous float64 array of nx*ny*3")
        ptr = accum.ctypes.data_as(C.c_void_p)
    else:
        import torch
        if accum.dtype != torch.float64 or accum.numel() != nx * ny * 3 or not accum.is_contiguous():
            raise ValueError("accum must be a contiguous float64 tensor of nx*ny*3")
        if not accum.is_cuda or accum.device.index != scenes[0].device:
            raise ValueError(f"a torch accum must live on scenes[0]'s GPU (cuda:{scenes[0].device})")
        torch.cuda.synchronize(accum.device)
        ptr = C.c_void_p(accum.data_ptr())
        on_device = 1
    handles = (C.c_void_p * len(scenes))(*[s.handle.value for s in scenes])
    prm = _abi.rtw_render_params(nx=nx, ny=ny, spp=spp, max_depth=max_depth, seed=seed, spp_begin=spp_begin,
                                 spp_count=spp_count, row_begin=row_begin, row_step=row_step,
                                 accum_on_device=on_device, collect_kernel_times=int(collect_kernel_times),
                                 wavefront_paths=0, precision=_precision(precision))
    st = _abi.rtw_stats()
    cam = camera if camera is not None else scenes[0].scene.camera
    check(lib().rtw_render_multi(len(scenes), handles, C.byref(cam), C.byref(prm), ptr, C.byref(st)),
          "rtw_render_multi")
    return accum, st.as_dict()


def _precision(name: str) -> int:
    try:
        return _abi.PRECISIONS[name]
    except KeyError:
        raise ValueError(f"precision must be one of {sorted(_abi.PRECISIONS)}, not {name!r}") from None


def write_ppm_quantized(path: str, rgb: np.ndarray, nx: int, ny: int) -> None:
    q = np.ascontiguousarray(rgb, dtype=np.int32)
    check(lib().rtw_write_ppm_quantized(str(path).encode(), q.ctypes.data_as(C.c_void_p), nx, ny),
          "rtw_write_ppm_quantized")


def build_id() -> str:
    return lib().rtw_build_id().decode()


def device_count() -> int:
    return lib().rtw_device_count()


def finalize(accum: np.ndarray, nx: int, ny: int, spp: int) -> np.ndarray:
    """canvas = min(sqrt(sum / spp), 1) (RayTracingWeekend.cpp:241-244), via the
    library's rtw_finalize_canvas."""
    return _finalize(accum, nx, ny, n=spp)


def _finalize(sums, nx: int, ny: int, n=None, counts=None) -> np.ndarray:
    """The host canvas of channel sums over `n` samples (unchecked, as the
    reference's), over counts[p], or of a mean (neither)."""
    a = np.ascontiguousarray(sums, dtype=np.float64)
    c = np.ascontiguousarray(counts, dtype=np.uint32) if counts is not None else None
    if n is None and (a.size != nx * ny * 3 or (c is not None and c.size != nx * ny)):
        raise ValueError("the sums (or the mean) must hold nx*ny*3 values and counts nx*ny")
    out = np.empty(nx * ny * 3, dtype=np.float64)
    pa, po = a.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    if c is not None:
        check(lib().rtw_finalize_canvas_counts(pa, c.ctypes.data_as(C.c_void_p), nx, ny, po),
              "rtw_finalize_canvas_counts")
    elif n is not None:
        lib().rtw_finalize_canvas(pa, nx, ny, n, po)
    else:
        check(lib().rtw_finalize_canvas_mean(pa, nx, ny, po), "rtw_finalize_canvas_mean")
    return out


def _zeros_like(a):
    if isinstance(a, np.ndarray):
        return np.zeros_like(a)
    import torch
    return torch.zeros_like(a)


def noise_estimate(accum: np.ndarray, accum_sq: np.ndarray, nx: int, ny: int, n: int, floor: float = 1e-2,
                   want_stderr: bool = True):
    """rtw_noise_estimate on the host: from the raw moments of `n` samples per
    pixel (DeviceScene.render_moments) the standard error of every channel's
    mean and the image-wide summary {pixels, nonfinite, mean_rel, max_rel,
    rms_stderr} (include/rtw_noise.h).  Returns (stderr array or None,
    summary dict)."""
    return _noise_estimate(accum, accum_sq, nx, ny, floor, want_stderr, n=n)


def _noise_estimate(accum, accum_sq, nx: int, ny: int, floor: float, want_stderr: bool, n=None, counts=None):
    """The host estimate with `n` samples in every pixel, or counts[p]."""
    a = np.ascontiguousarray(accum, dtype=np.float64)
    q = np.ascontiguousarray(accum_sq, dtype=np.float64)
    if a.size != nx * ny * 3 or q.size != nx * ny * 3:
        raise ValueError("accum and accum_sq must hold nx*ny*3 values")
    se = np.empty(nx * ny * 3, dtype=np.float64) if want_stderr else None
    out = _abi.rtw_noise_summary()
    pa, pq = a.ctypes.data_as(C.c_void_p), q.ctypes.data_as(C.c_void_p)
    tail = (floor, se.ctypes.data_as(C.c_void_p) if want_stderr else None, C.byref(out))
    if counts is None:
        check(lib().rtw_noise_estimate(pa, pq, nx, ny, n, *tail), "rtw_noise_estimate")
    else:
        _, _, c = _moments_counts(a, q, counts, nx, ny)
        check(lib().rtw_noise_estimate_counts(pa, pq, c.ctypes.data_as(C.c_void_p), nx, ny, *tail),
              "rtw_noise_estimate_counts")
    return se, out.as_dict()


def render_to_noise(ds, nx: int, ny: int, max_spp: int, max_depth: int, seed: int = 0, *, target: float,
                    first_batch: int = 8, floor: float = 1e-2, precision: str = "fp64",
                    device_buffers: bool = False, camera=None) -> dict:
    """Render batches of samples until the image-wide noise estimate reaches
    `target`: the sample ranges [0,b) [b,2b) [2b,4b) ... (b = first_batch; the
    total doubles at every check, the last batch is cut at max_spp), each
    through ds.render_moments with spp = max_spp, and after each
    ds.noise_estimate's mean_rel.  Stops at the first check with
    mean_rel <= target, or at max_spp.  The RNG is keyed by (seed, pixel,
    sample), so the buffers are those of one render of [0, spp_done) (up to
    the rounding of adding the batches' sums).

    `ds` is a DeviceScene, or anything with its render_moments and
    noise_estimate.  device_buffers keeps both moments in torch tensors on the
    scene's GPU.  Returns a dict: accum, accum_sq, spp_done, reached, history
    (a list of (spp, mean_rel, max_rel)) and stats (summed over the batches).
    Finalize the canvas with spp_done."""
    if first_batch < 2:
        raise ValueError("first_batch must be at least 2 (a variance needs two samples)")
    if max_spp < 2:
        raise ValueError("max_spp must be at least 2")
    if not target > 0:
        raise ValueError("target must be positive")
    if device_buffers:
        import torch
        accum = torch.zeros(nx * ny * 3, dtype=torch.float64, device=f"cuda:{ds.device}")
        accum_sq = torch.zeros_like(accum)
    else:
        accum = np.zeros(nx * ny * 3, dtype=np.float64)
        accum_sq = np.zeros_like(accum)
    done, reached, history, stats = 0, False, [], {}
    while done < max_spp and not reached:
        count = min(first_batch if done == 0 else done, max_spp - done)
        _, _, st = ds.render_moments(nx, ny, max_spp, max_depth, seed, spp_begin=done, spp_count=count,
                                     accum=accum, accum_sq=accum_sq, camera=camera, precision=precision)
        for k, v in st.items():
            stats[k] = stats.get(k, 0) + v
        done += count
        _, summary = ds.noise_estimate(accum, accum_sq, nx, ny, done, floor, want_stderr=False)
        history.append((done, summary["mean_rel"], summary["max_rel"]))
        reached = summary["mean_rel"] <= target
    return {"accum": accum, "accum_sq": accum_sq, "spp_done": done, "reached": reached, "history": history,
            "stats": stats}


def _moments_counts(accum, accum_sq, counts, nx: int, ny: int):
    a = np.ascontiguousarray(accum, dtype=np.float64)
    q = np.ascontiguousarray(accum_sq, dtype=np.float64) if accum_sq is not None else None
    c = np.ascontiguousarray(counts, dtype=np.uint32)
    if a.size != nx * ny * 3 or (q is not None and q.size != nx * ny * 3) or c.size != nx * ny:
        raise ValueError("the moments must hold nx*ny*3 values and counts nx*ny")
    return a, q, c


def select_active(accum, accum_sq, counts, nx: int, ny: int, *, target_rel: float, max_count: int,
                  floor: float = 1e-2) -> np.ndarray:
    """rtw_adaptive_select on the host: the ascending uint32 list of the pixels
    with counts < max_count, finite moments and (counts < 2 or rel > target_rel)
    (include/rtw_adaptive.h)."""
    a, q, c = _moments_counts(accum, accum_sq, counts, nx, ny)
    out = np.empty(nx * ny, dtype=np.uint32)
    n = C.c_uint64()
    check(lib().rtw_adaptive_select(a.ctypes.data_as(C.c_void_p), q.ctypes.data_as(C.c_void_p),
                                    c.ctypes.data_as(C.c_void_p), nx, ny, floor, target_rel, max_count,
                                    out.ctypes.data_as(C.c_void_p), C.byref(n)), "rtw_adaptive_select")
    return out[:n.value].copy()


def select_active_window(accum, accum_sq, counts, nx: int, ny: int, *, target_rel: float, max_count: int, radius: int,
                         min_count: int = 0, floor: float = 1e-2) -> np.ndarray:
    """rtw_adaptive_select_window on the host: the ascending uint32 list of the
    pixels with min_count <= counts < max_count and finite moments in whose
    clipped (2*radius+1)^2 window some pixel is a source: finite, and
    counts < 2 or rel > target_rel (include/rtw_adaptive_window.h)."""
    a, q, c = _moments_counts(accum, accum_sq, counts, nx, ny)
    out = np.empty(nx * ny, dtype=np.uint32)
    n = C.c_uint64()
    check(lib().rtw_adaptive_select_window(a.ctypes.data_as(C.c_void_p), q.ctypes.data_as(C.c_void_p),
                                           c.ctypes.data_as(C.c_void_p), nx, ny, floor, target_rel, min_count,
                                           max_count, radius, out.ctypes.data_as(C.c_void_p), C.byref(n)),
          "rtw_adaptive_select_window")
    return out[:n.value].copy()


def noise_estimate_counts(accum, accum_sq, counts, nx: int, ny: int, floor: float = 1e-2, want_stderr: bool = True):
    """rtw_noise_estimate_counts on the host: noise_estimate with each pixel's
    own sample count; pixels with fewer than two samples are left out (counted
    in `nonfinite`).  Returns (stderr array or None, summary dict)."""
    return _noise_estimate(accum, accum_sq, nx, ny, floor, want_stderr, counts=counts)


def finalize_counts(accum, counts, nx: int, ny: int) -> np.ndarray:
    """canvas = min(sqrt(sum / counts[p]), 1) via rtw_finalize_canvas_counts."""
    return _finalize(accum, nx, ny, counts=counts)


def _adaptive_params(target_rel: float, floor: float, min_spp: int, max_spp: int, batch: int):
    if min_spp < 2:
        raise ValueError("min_spp must be at least 2 (a variance needs two samples)")
    if max_spp < min_spp:
        raise ValueError("max_spp must be at least min_spp")
    if batch < 0:
        raise ValueError("batch must not be negative (0: each round doubles the samples)")
    if not target_rel >= 0:
        raise ValueError("target_rel must not be negative")
    if not floor > 0:
        raise ValueError("floor must be positive")
    return _abi.rtw_adaptive_params(target_rel=target_rel, floor=floor, min_spp=min_spp, max_spp=max_spp, batch=batch)


def adaptive_schedule(min_spp: int, max_spp: int, batch: int = 0):
    """Every round's (begin, count) of the adaptive loop, from the library's
    rtw_adaptive_next_round: [0, min_spp), then `batch` samples a round
    (batch 0: as many as are done, doubling), the last cut at max_spp."""
    ap = _adaptive_params(0.0, 1.0, min_spp, max_spp, batch)
    rounds, done = [], 0
    while True:
        b, c = C.c_int(), C.c_int()
        check(lib().rtw_adaptive_next_round(C.byref(ap), done, C.byref(b), C.byref(c)), "rtw_adaptive_next_round")
        if c.value == 0:
            return rounds
        rounds.append((b.value, c.value))
        done = b.value + c.value


def render_adaptive(ds, nx: int, ny: int, max_spp: int, max_depth: int, seed: int = 0, *, target_rel: float,
                    min_spp: int = 16, batch: int = 0, floor: float = 1e-2, precision: str = "fp64",
                    device_buffers: bool = False, camera=None, denoise: bool = False,
                    denoise_args: Optional[dict] = None, window: int = 0) -> dict:
    """Adaptive per-pixel sampling, the library's loop (rtw_render_adaptive):
    [0, min_spp) of every pixel, then rounds of `batch` samples (0: doubling)
    of the pixels whose relative standard error is still above target_rel,
    until none is or max_spp samples are done.  A pixel stopped on the variance
    of its own samples is biased low where it is dark and heavy-tailed: that
    is what min_spp is for (include/rtw_adaptive.h).

    window=R > 0 (at most 16) runs rtw_render_adaptive_window instead: a pixel
    keeps sampling while any pixel within R pixels of it is still above
    target_rel, which lessens that bias at the cost of more samples
    (include/rtw_adaptive_window.h); 0 is rtw_render_adaptive itself.

    Returns a dict: accum, accum_sq (float64), counts (uint32 array, or int32
    tensor with device_buffers), rounds, samples, pixels_at_max, summary
    (noise_estimate_counts of the result), history (per round: (begin, count,
    pixels rendered), read from the schedule and the counts) and stats.

    denoise=True additionally renders the first-hit features of the samples
    [0, min_spp) every pixel took and filters the moments with the per-pixel
    counts (ds.denoise, rtw_denoise.h; denoise_args: its parameters): the
    dict gains features, feature_spp and denoised (the linear mean; finalize
    it with ds.finalize_mean)."""
    ap = _adaptive_params(target_rel, floor, min_spp, max_spp, batch)
    if not 0 <= window <= _abi.RTW_WINDOW_RADIUS_MAX:
        raise ValueError(f"window must lie in [0, {_abi.RTW_WINDOW_RADIUS_MAX}]")
    if device_buffers:
        import torch
        accum = torch.zeros(nx * ny * 3, dtype=torch.float64, device=f"cuda:{ds.device}")
        accum_sq = torch.zeros_like(accum)
        counts = torch.zeros(nx * ny, dtype=torch.int32, device=accum.device)
        torch.cuda.synchronize(accum.device)
        ptrs = [C.c_void_p(t.data_ptr()) for t in (accum, accum_sq, counts)]
    else:
        accum = np.zeros(nx * ny * 3, dtype=np.float64)
        accum_sq = np.zeros_like(accum)
        counts = np.zeros(nx * ny, dtype=np.uint32)
        ptrs = [a.ctypes.data_as(C.c_void_p) for a in (accum, accum_sq, counts)]
    prm = _abi.rtw_render_params(nx=nx, ny=ny, spp=max_spp, max_depth=max_depth, seed=seed, row_step=1,
                                 accum_on_device=int(device_buffers), precision=_precision(precision))
    res, st = _abi.rtw_adaptive_result(), _abi.rtw_stats()
    cam = camera if camera is not None else ds.scene.camera
    if window:
        check(lib().rtw_render_adaptive_window(ds.handle, C.byref(cam), C.byref(prm), C.byref(ap), window, *ptrs,
                                               C.byref(res), C.byref(st)), "rtw_render_adaptive_window")
    else:
        check(lib().rtw_render_adaptive(ds.handle, C.byref(cam), C.byref(prm), C.byref(ap), *ptrs, C.byref(res),
                                        C.byref(st)), "rtw_render_adaptive")
    c_host = counts if isinstance(counts, np.ndarray) else counts.cpu().numpy()
    history = [(b, c, int((c_host > b).sum())) for b, c in adaptive_schedule(min_spp, max_spp, batch)[:res.rounds]]
    out = {"accum": accum, "accum_sq": accum_sq, "counts": counts, "rounds": res.rounds, "samples": res.samples,
           "pixels_at_max": res.pixels_at_max, "summary": res.final.as_dict(), "history": history,
           "stats": st.as_dict()}
    if denoise:
        features = _feature_zeros(nx, ny, ds.device if device_buffers else None)
        ds.render_features(nx, ny, max_spp, seed, spp_begin=0, spp_count=min_spp, features=features, camera=camera)
        out["features"], out["feature_spp"] = features, min_spp
        out["denoised"] = ds.denoise(accum, accum_sq, features, nx, ny, counts=counts, feature_spp=min_spp,
                                     **(denoise_args or {}))
    return out


def _feature_zeros(nx: int, ny: int, device: Optional[int]):
    n = nx * ny * _abi.RTW_FEATURE_CHANNELS
    if device is None:
        return np.zeros(n, dtype=np.float64)
    import torch
    return torch.zeros(n, dtype=torch.float64, device=f"cuda:{device}")


def denoise_params(**params) -> _abi.rtw_denoise_params:
    """rtw_denoise_default_params with `params` (iterations, sigma_l, sigma_z,
    eps_a, normal_power_log2) written over the defaults."""
    prm = _abi.rtw_denoise_params()
    lib().rtw_denoise_default_params(C.byref(prm))
    for k, v in params.items():
        if k not in ("iterations", "sigma_l", "sigma_z", "eps_a", "normal_power_log2"):
            raise ValueError(f"unknown denoise parameter {k!r}")
        setattr(prm, k, v)
    return prm


def denoise(accum, accum_sq, features, nx: int, ny: int, *, n: int = 0, counts=None, feature_spp: int,
            want_variance: bool = False, **params):
    """rtw_denoise on the host: the variance-guided edge-avoiding a-trous
    filter (include/rtw_denoise.h) of the raw moments of `n` samples per pixel
    (or a uint32 `counts` per pixel) guided by the first-hit feature sums of
    `feature_spp` samples per pixel (DeviceScene.render_features).  Returns
    the denoised linear mean (nx*ny*3), or (mean, variance) with
    want_variance."""
    a = np.ascontiguousarray(accum, dtype=np.float64)
    q = np.ascontiguousarray(accum_sq, dtype=np.float64)
    f = np.ascontiguousarray(features, dtype=np.float64)
    c = np.ascontiguousarray(counts, dtype=np.uint32) if counts is not None else None
    if a.size != nx * ny * 3 or q.size != nx * ny * 3 or f.size != nx * ny * _abi.RTW_FEATURE_CHANNELS \
            or (c is not None and c.size != nx * ny):
        raise ValueError("the moments must hold nx*ny*3 values, the features nx*ny*8 and counts nx*ny")
    out = np.empty(nx * ny * 3, dtype=np.float64)
    var = np.empty(nx * ny * 3, dtype=np.float64) if want_variance else None
    prm = denoise_params(**params)
    check(lib().rtw_denoise(a.ctypes.data_as(C.c_void_p), q.ctypes.data_as(C.c_void_p),
                            c.ctypes.data_as(C.c_void_p) if c is not None else None, n,
                            f.ctypes.data_as(C.c_void_p), feature_spp, nx, ny, C.byref(prm),
                            out.ctypes.data_as(C.c_void_p), var.ctypes.data_as(C.c_void_p) if want_variance else None),
          "rtw_denoise")
    return (out, var) if want_variance else out


def finalize_mean(mean, nx: int, ny: int) -> np.ndarray:
    """canvas = min(sqrt(mean), 1) via rtw_finalize_canvas_mean."""
    return _finalize(mean, nx, ny)


def render_denoised(ds, nx: int, ny: int, spp: int, max_depth: int, seed: int = 0, *, precision: str = "fp64",
                    device_buffers: bool = False, camera=None, **params) -> dict:
    """Render `spp` samples' moments and first-hit features, then filter
    (rtw_denoise.h).  Returns a dict: accum, accum_sq, features, denoised (the
    linear mean), canvas (min(sqrt(denoised), 1)) and stats (of the render)."""
    if spp < 2:
        raise ValueError("spp must be at least 2 (a variance needs two samples)")
    accum = accum_sq = None
    if device_buffers:
        import torch
        accum = torch.zeros(nx * ny * 3, dtype=torch.float64, device=f"cuda:{ds.device}")
        accum_sq = torch.zeros_like(accum)
    accum, accum_sq, stats = ds.render_moments(nx, ny, spp, max_depth, seed, accum=accum, accum_sq=accum_sq,
                                               camera=camera, precision=precision)
    features = _feature_zeros(nx, ny, ds.device if device_buffers else None)
    ds.render_features(nx, ny, spp, seed, features=features, camera=camera)
    den = ds.denoise(accum, accum_sq, features, nx, ny, n=spp, feature_spp=spp, **params)
    return {"accum": accum, "accum_sq": accum_sq, "features": features, "denoised": den,
            "canvas": ds.finalize_mean(den, nx, ny), "stats": stats}


def write_ppm(path: str, canvas: np.ndarray, nx: int, ny: int) -> None:
    c = np.ascontiguousarray(canvas, dtype=np.float64)
    check(lib().rtw_write_ppm(str(path).encode(), c.ctypes.data_as(C.c_void_p), nx, ny), "rtw_write_ppm")


def render(scene: str, nx: int, ny: int, spp: int, max_depth: int, seed: int = 0, device: int = 0,
           use_bvh: bool = False, **kw) -> Tuple[np.ndarray, dict]:
    """Render `scene` at nx*ny*spp on one GPU; returns (canvas, stats)."""
    sd = SceneDesc(scene, nx * 1.0 / ny, use_bvh)
    ds = DeviceScene(sd, device)
    try:
        accum, stats = ds.render_accumulate(nx, ny, spp, max_depth, seed, **kw)
    finally:
        ds.close()
    return finalize(accum, nx, ny, spp), stats
