"""Host-side binding of the HIP backend (mc_slam_amd/csrc/libvislam_ba.so) through its C-ABI.

There is NO CPU fallback: if the shared library is missing or no HIP device is present, construction
fails loudly.  The library is built in-tree by `python -c "import __graft_entry__ as g; g.build()"`
(or `make -C mc_slam_amd/csrc`).
"""
import ctypes as C
import os

from . import abi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("VBA_LIB", os.path.join(_HERE, "csrc", "libvislam_ba.so"))   # VBA_LIB: A/B builds in experiments
# the same library built with -DVBA_TEST_HOOKS (vba_debug_*: test / diagnostic hooks that the shipped library does not export)
HOOKS_LIB_PATH = os.environ.get("VBA_LIB", os.path.join(_HERE, "csrc", "libvislam_ba_hooks.so"))
_lib = None
_libs = {}

EXPORTS = ["vba_create", "vba_destroy", "vba_last_error", "vba_solve", "vba_batch_upload", "vba_batch_run",
           "vba_batch_download", "vba_batch_solve", "vba_solve_b", "vba_batch_run_b", "vba_batch_solve_b", "vba_preintegrate", "vba_pose_optimize", "vba_problem_save", "vba_problem_load", "vba_problem_free", "vba_set_profile", "vba_get_profile", "vba_host_threads",
           "vba_batch_set_depth", "vba_batch_submit", "vba_batch_submit_b", "vba_batch_poll", "vba_batch_wait", "vba_sim3_optimize",
           "vba_posegraph_optimize", "vba_sim3_ransac", "vba_triangulate", "vba_two_view_init", "vba_search_triangulation", "vba_fuse",
           "vba_search_by_sim3", "vba_search_by_projection", "vba_search_by_bow", "vba_search_by_projection_kf",
           "vba_search_for_initialization", "vba_mappoint_update"]

# The small-problem entry points, all of the shape fn(handle, n, problems, results).  kind -> (library function, problem struct,
# result struct, result buffer of one problem -- called with the problem and the extra arguments of its pack --, whether the call
# works on private copies of the problems)
_SMALL = {
    "pose": ("vba_pose_optimize", abi.vba_frame_problem, abi.vba_frame_result, abi.FrameResultBuf, False),
    "sim3": ("vba_sim3_optimize", abi.vba_sim3_problem, abi.vba_sim3_result, abi.Sim3ResultBuf, False),
    "sim3_ransac": ("vba_sim3_ransac", abi.vba_sim3_ransac_problem, abi.vba_sim3_ransac_result, abi.Sim3RansacResultBuf, False),
    "triangulate": ("vba_triangulate", abi.vba_triangulate_problem, abi.vba_triangulate_result, abi.TriangulateResultBuf, False),
    "two_view": ("vba_two_view_init", abi.vba_two_view_problem, abi.vba_two_view_result, abi.TwoViewResultBuf, False),
    "search_triangulation": ("vba_search_triangulation", abi.vba_search_tri_problem, abi.vba_search_tri_result, abi.SearchTriResultBuf, False),
    "fuse": ("vba_fuse", abi.vba_fuse_problem, abi.vba_fuse_result, abi.FuseResultBuf, False),
    "search_by_sim3": ("vba_search_by_sim3", abi.vba_search_sim3_problem, abi.vba_search_sim3_result, abi.SearchSim3ResultBuf, False),
    "search_by_projection": ("vba_search_by_projection", abi.vba_search_proj_problem, abi.vba_search_proj_result, abi.SearchProjResultBuf, False),
    "search_by_projection_kf": ("vba_search_by_projection_kf", abi.vba_search_proj_kf_problem, abi.vba_search_proj_kf_result, abi.SearchProjKfResultBuf,
                                False),
    "search_by_bow": ("vba_search_by_bow", abi.vba_search_bow_problem, abi.vba_search_bow_result, abi.SearchBowResultBuf, False),
    "search_for_initialization": ("vba_search_for_initialization", abi.vba_search_init_problem, abi.vba_search_init_result, abi.SearchInitResultBuf,
                                  False),
    "mappoint_update": ("vba_mappoint_update", abi.vba_mappoint_problem, abi.vba_mappoint_result, abi.MapPointResultBuf, False),
    "posegraph": ("vba_posegraph_optimize", abi.vba_posegraph_problem, abi.vba_posegraph_result, lambda p: abi.vba_posegraph_result(), True),
}


def load_library(hooks=False):
    """dlopen the in-tree HIP library and declare every entry point of include/vislam_ba.h.  hooks=True: the flavour with the
    test / diagnostic hooks (a second, independent instance of the library)."""
    global _lib
    path = HOOKS_LIB_PATH if hooks else LIB_PATH
    if path in _libs:
        return _libs[path]
    if not os.path.exists(path):
        raise RuntimeError("HIP backend not built: %s is missing (run __graft_entry__.build())" % path)
    lib = C.CDLL(path)
    PP = C.POINTER(C.POINTER(abi.vba_problem))
    PR = C.POINTER(C.POINTER(abi.vba_result))
    lib.vba_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    lib.vba_destroy.argtypes = [C.c_void_p]
    lib.vba_last_error.argtypes = [C.c_void_p]
    lib.vba_last_error.restype = C.c_char_p
    lib.vba_solve.argtypes = [C.c_void_p, C.POINTER(abi.vba_problem), C.POINTER(abi.vba_result), C.c_void_p]
    lib.vba_batch_upload.argtypes = [C.c_void_p, C.c_int32, PP]
    lib.vba_batch_run.argtypes = [C.c_void_p, C.c_void_p]
    lib.vba_batch_download.argtypes = [C.c_void_p, C.c_int32, PP, PR]
    lib.vba_batch_solve.argtypes = [C.c_void_p, C.c_int32, PP, PR, C.c_void_p]
    lib.vba_solve_b.argtypes = [C.c_void_p, C.POINTER(abi.vba_problem), C.POINTER(abi.vba_result), C.c_void_p]
    lib.vba_batch_run_b.argtypes = [C.c_void_p, C.c_void_p]
    lib.vba_batch_solve_b.argtypes = [C.c_void_p, C.c_int32, PP, PR, C.c_void_p]
    _pd, _pi = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    lib.vba_preintegrate.argtypes = [C.c_void_p, C.c_int32, _pi, _pd, _pd, _pd, C.c_double, C.c_double, _pd, _pd, _pd]
    for fn, problem, result, _, _ in _SMALL.values():
        getattr(lib, fn).argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.POINTER(problem)), C.POINTER(C.POINTER(result))]
    lib.vba_set_profile.argtypes = [C.c_void_p, C.c_int32]
    lib.vba_get_profile.argtypes = [C.c_void_p, C.POINTER(abi.vba_profile)]
    lib.vba_batch_set_depth.argtypes = [C.c_void_p, C.c_int32]
    lib.vba_batch_submit.argtypes = [C.c_void_p, C.c_int32, PP, PR, C.c_void_p, C.POINTER(C.c_int64)]
    lib.vba_batch_submit_b.argtypes = [C.c_void_p, C.c_int32, PP, PR, C.c_void_p, C.POINTER(C.c_int64)]
    lib.vba_batch_poll.argtypes = [C.c_void_p, C.c_int64]
    lib.vba_batch_wait.argtypes = [C.c_void_p, C.c_int64]
    if hooks:
        lib.vba_debug_async_hold.argtypes = [C.c_void_p, C.c_int32]
        lib.vba_debug_posegraph_system.argtypes = [C.c_void_p, C.POINTER(abi.vba_posegraph_problem), _pd, _pd, _pd]
        lib.vba_debug_posegraph_system.restype = C.c_int
    for n in EXPORTS:
        if n != "vba_last_error":
            getattr(lib, n).restype = C.c_int
    _libs[path] = lib
    if not hooks:
        _lib = lib
    return lib


class LocalBA:
    """One backend handle = one GPU + one stream (vba_create).  Mirrors how the reference owns one
    function-local g2o::SparseOptimizer per call (src/Optimizer.cpp:130), but keeps device buffers alive."""

    def __init__(self, device=0, hooks=False):
        self.lib = load_library(hooks)
        self.h = C.c_void_p()
        rc = self.lib.vba_create(device, C.byref(self.h))
        if rc != 0:
            raise RuntimeError("vba_create(device=%d) failed (rc=%d): no usable HIP device -- the backend has no CPU path"
                               % (device, rc))
        self._keep = None
        self._tickets = {}   # ticket -> (packed copies, stop flag): what the library reads until the ticket is retired

    def close(self):
        if self.h:
            for t in sorted(getattr(self, "_tickets", {})):   # pending batches finish first: their results land in the packed copies
                self.lib.vba_batch_wait(self.h, t)
            self.lib.vba_destroy(self.h)
            self.h = C.c_void_p()
            self._tickets = {}

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _err(self, what):
        return RuntimeError("%s: %s" % (what, self.lib.vba_last_error(self.h).decode()))

    @staticmethod
    def _stop_ptr(stop):
        return C.cast(C.pointer(stop), C.c_void_p) if stop is not None else None

    def solve(self, prob: abi.Problem, stop=None):
        """vba_solve on a COPY of prob: returns (solved copy, Result)."""
        q = prob.copy()
        s = q.as_struct()
        rb = abi.ResultBuf(q.n_obs)
        if self.lib.vba_solve(self.h, C.byref(s), C.byref(rb.s), self._stop_ptr(stop)) != 0:
            raise self._err("vba_solve")
        return q, rb.get()

    # ---- device-resident batch interface -------------------------------------------------------
    def upload(self, probs):
        self._probs = [p.copy() for p in probs]
        self._structs = [p.as_struct() for p in self._probs]
        n = len(probs)
        arr = (C.POINTER(abi.vba_problem) * n)(*[C.pointer(s) for s in self._structs])
        self._parr = arr
        if self.lib.vba_batch_upload(self.h, n, arr) != 0:
            raise self._err("vba_batch_upload")

    def run(self, stop=None):
        if self.lib.vba_batch_run(self.h, self._stop_ptr(stop)) != 0:
            raise self._err("vba_batch_run")

    def download(self):
        n = len(self._probs)
        rbs = [abi.ResultBuf(p.n_obs) for p in self._probs]
        rarr = (C.POINTER(abi.vba_result) * n)(*[C.pointer(r.s) for r in rbs])
        if self.lib.vba_batch_download(self.h, n, self._parr, rarr) != 0:
            raise self._err("vba_batch_download")
        return self._probs, [r.get() for r in rbs]

    # ---- fresh windows in, solved windows out (vba_batch_solve: chunks of the batch in flight concurrently) ----
    def pack(self, probs, want_chi2=True):
        """private copies of the windows + the ctypes views vba_batch_solve needs (kept alive by the returned dict)"""
        n = len(probs)
        own = [p.copy() for p in probs]
        structs = [p.as_struct() for p in own]
        rbs = [abi.ResultBuf(p.n_obs, want_chi2) for p in own]
        return dict(n=n, src=list(probs), own=own, structs=structs, rbs=rbs,
                    parr=(C.POINTER(abi.vba_problem) * n)(*[C.pointer(s) for s in structs]),
                    rarr=(C.POINTER(abi.vba_result) * n)(*[C.pointer(r.s) for r in rbs]))

    @staticmethod
    def pack_reset(packed):
        """the solve updates the states in place: put the initial states back (outside any timed region)"""
        for q, p in zip(packed["own"], packed["src"]):
            for k in ("kf_pose", "kf_vel", "kf_bias", "pt"):
                getattr(q, k)[...] = getattr(p, k)

    def solve_packed(self, packed, stop=None):
        if self.lib.vba_batch_solve(self.h, packed["n"], packed["parr"], packed["rarr"], self._stop_ptr(stop)) != 0:
            raise self._err("vba_batch_solve")

    @staticmethod
    def pack_results(packed):
        return packed["own"], [r.get() for r in packed["rbs"]]

    def solve_batch(self, probs, stop=None):
        """vba_batch_solve on copies of probs: (solved copies, Results)"""
        packed = self.pack(probs)
        self.solve_packed(packed, stop)
        return self.pack_results(packed)

    # ---- asynchronous batches (vba_batch_submit / poll / wait): batch k+1 is handed over while batch k solves ----
    def submit_packed(self, packed, stop=None):
        """vba_batch_submit of a pack(): returns the ticket.  The packed copies and the stop flag stay referenced by this object
        until the ticket is retired (wait); stop: a one-byte ctypes flag (c_uint8, c_bool) goes through vba_batch_submit_b."""
        t = C.c_int64(0)
        fn = self.lib.vba_batch_submit_b if stop is not None and C.sizeof(stop) == 1 else self.lib.vba_batch_submit
        if fn(self.h, packed["n"], packed["parr"], packed["rarr"], self._stop_ptr(stop), C.byref(t)) != 0:
            raise self._err("vba_batch_submit")
        self._tickets[t.value] = (packed, stop)
        return t.value

    def submit(self, probs, stop=None, want_chi2=True):
        """vba_batch_submit on private copies of probs (pack): returns the ticket; wait(ticket) hands the solved copies back"""
        return self.submit_packed(self.pack(probs, want_chi2), stop)

    def poll(self, ticket):
        """True once the ticket has finished (wait will not block), False while it is pending"""
        rc = self.lib.vba_batch_poll(self.h, ticket)
        if rc < 0:
            raise self._err("vba_batch_poll")
        return rc == 0

    def wait_packed(self, ticket):
        """vba_batch_wait: retires the ticket and returns its pack() (results in place); RuntimeError if the batch failed"""
        rc = self.lib.vba_batch_wait(self.h, ticket)
        packed = self._tickets.pop(ticket, (None, None))[0]
        if rc != 0:
            raise self._err("vba_batch_wait")
        return packed

    def wait(self, ticket):
        """vba_batch_wait: (solved copies, Results) of the ticket"""
        return self.pack_results(self.wait_packed(ticket))

    def set_depth(self, n):
        """vba_batch_set_depth: batches resident on the device at once (1..4)"""
        if self.lib.vba_batch_set_depth(self.h, n) != 0:
            raise self._err("vba_batch_set_depth")

    def preintegrate(self, sample_begin, gyr, acc, dt, want_info=True):
        """vba_preintegrate: (imu_meas [E,61], cov_PVphi [E,9,9], info_PphiV [E,9,9] or None)"""
        import numpy as np
        sb = np.ascontiguousarray(sample_begin, dtype=np.int32)
        g = np.ascontiguousarray(gyr, dtype=np.float64).reshape(-1, 3)
        a = np.ascontiguousarray(acc, dtype=np.float64).reshape(-1, 3)
        d = np.ascontiguousarray(dt, dtype=np.float64)
        E = len(sb) - 1
        meas = np.zeros((E, abi.IMU_MEAS_STRIDE)); cov = np.zeros((E, 81)); info = np.zeros((E, 81))
        P = lambda x, t: x.ctypes.data_as(C.POINTER(t))
        rc = self.lib.vba_preintegrate(self.h, E, P(sb, C.c_int32), P(g, C.c_double), P(a, C.c_double), P(d, C.c_double),
                                       abi.GYR_MEAS_COV, abi.ACC_MEAS_COV, P(meas, C.c_double), P(cov, C.c_double),
                                       P(info, C.c_double) if want_info else None)
        if rc != 0:
            raise self._err("vba_preintegrate")
        return meas, cov.reshape(E, 9, 9), (info.reshape(E, 9, 9) if want_info else None)

    # ---- the small-problem entry points: a batch of independent problems per call.  <topic>_pack makes the ctypes views once,
    # <topic>_call runs the library on them (again and again in a benchmark), <topic>_reset puts back what a call updated in place
    @staticmethod
    def _small_pack(kind, problems, *buf_args):
        """(n, problem structs, result buffers, the two pointer arrays, problems[, private copies]): the ctypes views of a list of
        the kind's abi problems, kept alive by the returned tuple"""
        _, problem, result, make_buf, copied = _SMALL[kind]
        n = len(problems)
        own = [p.copy() for p in problems] if copied else problems
        structs = [p.as_struct() for p in own]
        bufs = [make_buf(p, *buf_args) for p in own]
        pp = (C.POINTER(problem) * n)(*[C.pointer(s) for s in structs])
        rr = (C.POINTER(result) * n)(*[C.pointer(getattr(b, "s", b)) for b in bufs])
        return (n, structs, bufs, pp, rr, problems) + ((own,) if copied else ())

    def _small_call(self, kind, packed):
        fn = _SMALL[kind][0]
        if getattr(self.lib, fn)(self.h, packed[0], packed[3], packed[4]) != 0:
            raise self._err(fn)

    # vba_pose_optimize: abi.FrameProblem
    def pose_pack(self, frames):
        return self._small_pack("pose", frames)

    def pose_reset(self, packed):
        """vba_pose_optimize updates nav in place: put the frames' initial states back before the next run"""
        for s, f in zip(packed[1], packed[5]):
            C.memmove(C.addressof(s) + abi.vba_frame_problem.nav.offset, f.nav.ctypes.data, 8 * abi.NAV_STRIDE)

    def pose_call(self, packed):
        self._small_call("pose", packed)

    def pose_run(self, packed):
        self.pose_reset(packed)
        self.pose_call(packed)

    def pose_optimize(self, frames):
        """vba_pose_optimize on copies of the FrameProblems: list of abi.FrameResult (with the optimised nav)"""
        packed = self.pose_pack(frames)
        self.pose_run(packed)
        return [b.get(s) for b, s in zip(packed[2], packed[1])]

    # loop-closure Sim3 refinement (vba_sim3_optimize): abi.Sim3Problem
    def sim3_pack(self, problems, want_chi2=True):
        return self._small_pack("sim3", problems, want_chi2)

    def sim3_reset(self, packed):
        """vba_sim3_optimize updates S12 in place: put the initial estimates back before the next run"""
        for s, p in zip(packed[1], packed[5]):
            C.memmove(C.addressof(s) + abi.vba_sim3_problem.S12.offset, p.S12.ctypes.data, 64)

    def sim3_call(self, packed):
        self._small_call("sim3", packed)

    def sim3_optimize(self, problems, want_chi2=True):
        """vba_sim3_optimize on a list of abi.Sim3Problem (left untouched): list of abi.Sim3Result with the refined S12"""
        packed = self.sim3_pack(problems, want_chi2)
        self.sim3_call(packed)
        return [b.get(s) for b, s in zip(packed[2], packed[1])]

    # loop-candidate Sim3 RANSAC (vba_sim3_ransac): abi.Sim3RansacProblem
    def sim3_ransac_pack(self, problems, want_counts=True):
        return self._small_pack("sim3_ransac", problems, want_counts)

    def sim3_ransac_reset(self, packed):
        """vba_sim3_ransac updates best_inliers / best_S12 in place: put the solvers' states back before the next run"""
        for s, p in zip(packed[1], packed[5]):
            s.best_inliers = int(p.best_inliers)
            s.best_S12[:] = p.best_S12.tolist()

    def sim3_ransac_call(self, packed):
        self._small_call("sim3_ransac", packed)

    def sim3_ransac(self, problems, want_counts=True):
        """vba_sim3_ransac on a list of abi.Sim3RansacProblem (left untouched): list of abi.Sim3RansacResult, each with the
        solver's state (best_inliers, best_S12) after the call"""
        packed = self.sim3_ransac_pack(problems, want_counts)
        self.sim3_ransac_call(packed)
        return [b.get(s) for b, s in zip(packed[2], packed[1])]

    # two-view triangulation of new map points (vba_triangulate): abi.TriangulateProblem, one keyframe pair each
    def triangulate_pack(self, problems):
        return self._small_pack("triangulate", problems)

    def triangulate_call(self, packed):
        self._small_call("triangulate", packed)

    def triangulate(self, problems):
        """vba_triangulate on a list of abi.TriangulateProblem: list of abi.TriangulateResult"""
        packed = self.triangulate_pack(problems)
        self.triangulate_call(packed)
        return [b.get() for b in packed[2]]

    # monocular two-view initialisation (vba_two_view_init): abi.TwoViewProblem, one frame pair each
    def two_view_pack(self, problems, want_scores=True, fill=0):
        return self._small_pack("two_view", problems, want_scores, fill)

    def two_view_call(self, packed):
        self._small_call("two_view", packed)

    def two_view_init(self, problems, want_scores=True, fill=0):
        """vba_two_view_init on a list of abi.TwoViewProblem: list of abi.TwoViewResult"""
        packed = self.two_view_pack(problems, want_scores, fill)
        self.two_view_call(packed)
        return [b.get() for b in packed[2]]

    # matching for triangulation (vba_search_triangulation): abi.SearchTriProblem, one keyframe pair each
    def search_triangulation_pack(self, problems):
        return self._small_pack("search_triangulation", problems)

    def search_triangulation_call(self, packed):
        self._small_call("search_triangulation", packed)

    def search_triangulation(self, problems):
        """vba_search_triangulation on a list of abi.SearchTriProblem: list of abi.SearchTriResult"""
        packed = self.search_triangulation_pack(problems)
        self.search_triangulation_call(packed)
        return [b.get() for b in packed[2]]

    # projection search for map-point fusion (vba_fuse): abi.FuseProblem, one keyframe and one point list each
    def fuse_pack(self, problems):
        return self._small_pack("fuse", problems)

    def fuse_call(self, packed):
        self._small_call("fuse", packed)

    def fuse(self, problems):
        """vba_fuse on a list of abi.FuseProblem: list of abi.FuseResult"""
        packed = self.fuse_pack(problems)
        self.fuse_call(packed)
        return [b.get() for b in packed[2]]

    # Sim3 projection matching for loop candidates (vba_search_by_sim3): abi.SearchSim3Problem, one keyframe pair each
    def search_by_sim3_pack(self, problems):
        return self._small_pack("search_by_sim3", problems)

    def search_by_sim3_call(self, packed):
        self._small_call("search_by_sim3", packed)

    def search_by_sim3(self, problems):
        """vba_search_by_sim3 on a list of abi.SearchSim3Problem: list of abi.SearchSim3Result"""
        packed = self.search_by_sim3_pack(problems)
        self.search_by_sim3_call(packed)
        return [b.get() for b in packed[2]]

    # projection matching for tracking (vba_search_by_projection): abi.SearchProjProblem, one frame and one ordered query list each
    def search_by_projection_pack(self, problems):
        return self._small_pack("search_by_projection", problems)

    def search_by_projection_call(self, packed):
        self._small_call("search_by_projection", packed)

    def search_by_projection(self, problems):
        """vba_search_by_projection on a list of abi.SearchProjProblem: list of abi.SearchProjResult"""
        packed = self.search_by_projection_pack(problems)
        self.search_by_projection_call(packed)
        return [b.get() for b in packed[2]]

    # projection matching for loop closure and relocalisation (vba_search_by_projection_kf): abi.SearchProjKfProblem, one target and
    # one ordered query list each, both modes mixed
    def search_by_projection_kf_pack(self, problems):
        return self._small_pack("search_by_projection_kf", problems)

    def search_by_projection_kf_call(self, packed):
        self._small_call("search_by_projection_kf", packed)

    def search_by_projection_kf(self, problems):
        """vba_search_by_projection_kf on a list of abi.SearchProjKfProblem: list of abi.SearchProjKfResult"""
        packed = self.search_by_projection_kf_pack(problems)
        self.search_by_projection_kf_call(packed)
        return [b.get() for b in packed[2]]

    # bag-of-words matching (vba_search_by_bow): abi.SearchBowProblem, one pair each, both modes mixed
    def search_by_bow_pack(self, problems):
        return self._small_pack("search_by_bow", problems)

    def search_by_bow_call(self, packed):
        self._small_call("search_by_bow", packed)

    def search_by_bow(self, problems):
        """vba_search_by_bow on a list of abi.SearchBowProblem: list of abi.SearchBowResult"""
        packed = self.search_by_bow_pack(problems)
        self.search_by_bow_call(packed)
        return [b.get() for b in packed[2]]

    # matching for the monocular initialisation (vba_search_for_initialization): abi.SearchInitProblem, one frame pair each
    def search_for_initialization_pack(self, problems):
        return self._small_pack("search_for_initialization", problems)

    def search_for_initialization_call(self, packed):
        self._small_call("search_for_initialization", packed)

    def search_for_initialization(self, problems):
        """vba_search_for_initialization on a list of abi.SearchInitProblem: list of abi.SearchInitResult"""
        packed = self.search_for_initialization_pack(problems)
        self.search_for_initialization_call(packed)
        return [b.get() for b in packed[2]]

    # map-point refresh (vba_mappoint_update): abi.MapPointProblem, one point list over one keyframe table each
    def mappoint_update_pack(self, problems):
        return self._small_pack("mappoint_update", problems)

    def mappoint_update_call(self, packed):
        self._small_call("mappoint_update", packed)

    def mappoint_update(self, problems):
        """vba_mappoint_update on a list of abi.MapPointProblem: list of abi.MapPointResult"""
        packed = self.mappoint_update_pack(problems)
        self.mappoint_update_call(packed)
        return [b.get() for b in packed[2]]

    # essential-graph optimisation (vba_posegraph_optimize): abi.PoseGraphProblem, independent Sim3 pose graphs.  The call updates
    # S and pt of the pack's private copies in place
    def posegraph_pack(self, problems):
        return self._small_pack("posegraph", problems)

    def posegraph_reset(self, packed):
        """put the initial estimates and points back before the next run"""
        for q, p in zip(packed[6], packed[5]):
            q.S[...] = p.S
            q.pt[...] = p.pt

    def posegraph_call(self, packed):
        self._small_call("posegraph", packed)

    def posegraph_optimize(self, problems):
        """vba_posegraph_optimize on copies of a list of abi.PoseGraphProblem: list of abi.PoseGraphResult"""
        packed = self.posegraph_pack(problems)
        self.posegraph_call(packed)
        return [abi.PoseGraphResult(r.status, r.its_done, r.lm_trials, r.stop, r.chi2_initial, r.chi2_final, r.lambda_final,
                                    q.S.copy(), q.pt.copy()) for r, q in zip(packed[2], packed[6])]

    def posegraph_system(self, problem):
        """hooks flavour: (H dense, b, x of the first trial of the first iteration) as k_posegraph_opt formed them"""
        import numpy as np
        q = problem.copy()
        s = q.as_struct()
        n = 7 * int((q.fixed == 0).sum())
        H, b, x = np.zeros((n, n)), np.zeros(n), np.zeros(n)
        P = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        if self.lib.vba_debug_posegraph_system(self.h, C.byref(s), P(H), P(b), P(x)) != 0:
            raise self._err("vba_debug_posegraph_system")
        return H, b, x

    def set_profile(self, on=True):
        self.lib.vba_set_profile(self.h, 1 if on else 0)

    def get_profile(self):
        pf = abi.vba_profile()
        self.lib.vba_get_profile(self.h, C.byref(pf))
        d = {abi.PROF_NAMES[i]: dict(ms=pf.ms[i], launches=pf.launches[i], bytes=pf.bytes[i]) for i in range(7)}
        d["factor"]["flops"] = pf.factor_flops
        d["total_ms"] = pf.total_ms
        d["kernel_launches"] = int(pf.kernel_launches)
        return d
