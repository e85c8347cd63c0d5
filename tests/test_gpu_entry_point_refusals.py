"""GPU: what the sweep, frame and image entry points of the C ABI answer to a call they refuse — status, vloam_last_error() and an
unchanged vloam_frame_count — and that a handle which refused all of them computes afterwards what a fresh handle computes.

The calls go through ctypes (the Python wrappers convert their arguments and would hide some cases).  Each call breaks exactly ONE rule, and
every bad argument is null, zero or a count: every non-null pointer points to memory of the stated size (host arrays of max_points + 1
points, device tensors of the same size, image buffers larger than any size named), because a call that is not refused reads it.

The expected answers are those of the library as it stood before the entry points were folded onto one admission path (commit e613bd3):
written down from its source, then checked by running this file against a build of that commit on an MI355X, where every one of them held
(profiles/c_api_entry_points.txt).  Two of them look wrong and are pinned all the same (vloam_vo_process_point_cloud answers an empty
cloud with VLOAM_ERR_INVALID and sets no message for either of its refusals).  Where a refusal sets no message, vloam_last_error() still holds the message of the refusal provoked just before
the call (SENTINEL)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MP = 4096          # max_points of the handles: one 16 x 256 sweep
IMG = 30           # 2 * kImgWin: the smallest image vloam_create accepts
VO_MAX = 8192      # kVoMaxMatches
SENTINEL = b"n_sessions must be 1..24"
ONE_SEQ = b"this entry point drives one sequence: the handle has 2 sessions (use the vloam_batch_* calls)"
TOO_BIG = b"cloud of 4097 points exceeds max_points=4096"
EMPTY = b"empty cloud"
NO_CALIB = b"vloam_process_frame needs vloam_vo_set_calib and vloam_set_extrinsics first"
NO_IMG = b"the handle was created without an image front-end (cfg.image_width / image_height)"
HOST_IMG = b"bad image size ("                    # + the sizes
DEV_IMG = b"image front-end: bad image size ("    # + the sizes
TOO_MANY = b"8193 matches exceed the capacity of 8192"


def null_sweep(b):
    return b"null sweep pointer for session %d" % b


def null_image(b):
    return b"null image pointer for session %d" % b


def bad_matches(b):
    return b"bad match arrays for session %d" % b


def vp(*vals):
    return (C.c_void_p * len(vals))(*vals)


def ci(*vals):
    return (C.c_int * len(vals))(*vals)


def swap(vals, b, v):
    out = list(vals)
    out[b] = v
    return out


class Inputs:
    """Valid arguments for every entry point: sweeps 0..2 for session 0 and 3..5 for session 1, in host and in device memory (one spare point
    behind each, so that n = max_points + 1 names memory that exists), a grey image, match arrays of kVoMaxMatches + 1 pairs."""

    def __init__(self, sweeps):
        import torch
        self.host = []
        for k in range(6):
            a = np.zeros((MP + 1, 4), np.float32)
            a[:MP] = sweeps(16, 256, k)
            self.host.append(a)
        self.dev = [torch.from_numpy(a).cuda() for a in self.host[:2]]
        self.gray = [np.zeros((64, 64), np.uint8) for _ in range(2)]
        self.dgray = [torch.zeros((64, 64), dtype=torch.uint8, device="cuda") for _ in range(2)]
        self.uv = [np.zeros((VO_MAX + 1, 2), np.int32) for _ in range(2)]
        torch.cuda.synchronize()


@pytest.fixture(scope="module")
def inputs(sweeps):
    return Inputs(sweeps)


def make_handle(vl, synth, B, with_image, calibrated=True):
    kw = dict(image_width=IMG, image_height=IMG) if with_image else {}
    hd = vl.Handle(0, n_sessions=B, scan_line=16, max_points=MP, max_frames=8, with_mapping=1, **kw)
    if calibrated:
        calibrate(hd, synth)
    return hd


def calibrate(hd, synth):
    hd.vo_set_calib(*synth.kitti_like_calib())
    hd.set_extrinsics(*synth.kitti_like_extrinsics())


def refusal_cases(L, h, B, with_image, inp, calibrated):
    """[(name, call, status, message, exact)] for one handle.  calibrated == False: only the frame calls that are refused for that reason."""
    INVALID, CAPACITY, EMPTY_ST, ORDER = -1, -3, -4, -6
    b = B - 1                                            # the session whose argument is broken in the batch calls
    hx, dx = [a.ctypes.data for a in inp.host[:B]], [t.data_ptr() for t in inp.dev[:B]]
    hg, dg = [g.ctypes.data for g in inp.gray[:B]], [t.data_ptr() for t in inp.dgray[:B]]
    uv = [u.ctypes.data for u in inp.uv[:B]]
    none, n_ok, zero = [None] * B, [MP] * B, [0] * B
    out = []

    def case(name, call, status, message=SENTINEL, exact=True):
        out.append((name, call, status, message, exact))

    # ---- the calls in their valid form, one argument list each; a case replaces one argument
    def scan1(fn, host):     # (h, cloud, n)
        x = (hx if host else dx)[0]
        return lambda hh=h, p=x, n=MP: getattr(L, fn)(hh, C.c_void_p(p), n)

    def scanB(fn, host):     # (h, clouds[], n[])
        x = hx if host else dx
        return lambda hh=h, p=x, n=n_ok, null_p=False, null_n=False: getattr(L, fn)(hh, None if null_p else vp(*p), None if null_n else ci(*n))

    def frame1(fn, host):    # (h, cloud, n, prev_uv, curr_uv, n_match)
        x = (hx if host else dx)[0]
        return lambda hh=h, p=x, n=MP, pu=None, cu=None, m=0: getattr(L, fn)(hh, C.c_void_p(p), n, C.c_void_p(pu), C.c_void_p(cu), m)

    def frameB(fn, host):    # (h, clouds[], n[], prev_uv[], curr_uv[], n_match[])
        x = hx if host else dx
        return lambda hh=h, p=x, n=n_ok, pu=none, cu=none, m=zero, null_p=False, null_n=False: getattr(L, fn)(
            hh, None if null_p else vp(*p), None if null_n else ci(*n), vp(*pu), vp(*cu), ci(*m))

    def image1(fn, host):    # (h, cloud, n, gray, width, height, stride)
        x, g0 = (hx if host else dx)[0], (hg if host else dg)[0]
        return lambda hh=h, p=x, n=MP, g=g0, w=IMG, ht=IMG, s=IMG: getattr(L, fn)(hh, C.c_void_p(p), n, C.c_void_p(g), w, ht, s)

    def imageB(fn, host):    # (h, clouds[], n[], grays[], width, height, stride)
        x, g0 = (hx if host else dx), (hg if host else dg)
        return lambda hh=h, p=x, n=n_ok, g=g0, w=IMG, ht=IMG, s=IMG, null_p=False, null_g=False, null_n=False: getattr(L, fn)(
            hh, None if null_p else vp(*p), None if null_n else ci(*n), None if null_g else vp(*g), w, ht, s)

    def voimg(fn, host):     # (h, gray, width, height, stride)
        g0 = (hg if host else dg)[0]
        return lambda hh=h, g=g0, w=IMG, ht=IMG, s=IMG: getattr(L, fn)(hh, C.c_void_p(g), w, ht, s)

    if not calibrated:
        if B == 1:
            for fn, host in (("vloam_process_frame", True), ("vloam_process_frame_device", False)):
                case(fn + ": no calibration", frame1(fn, host), ORDER, NO_CALIB)
            if with_image:
                for fn, host in (("vloam_process_frame_image", True), ("vloam_process_frame_image_device", False)):
                    case(fn + ": no calibration", image1(fn, host), ORDER, NO_CALIB)
        for fn, host in (("vloam_batch_process_frame", True), ("vloam_batch_process_frame_device", False)):
            case(fn + ": no calibration", frameB(fn, host), ORDER, NO_CALIB)
        if with_image:
            for fn, host in (("vloam_batch_process_frame_image", True), ("vloam_batch_process_frame_image_device", False)):
                case(fn + ": no calibration", imageB(fn, host), ORDER, NO_CALIB)
        return out

    def image_size_cases(fn, f, message):
        case(fn + ": width 0", lambda: f(w=0), INVALID, message, False)
        case(fn + ": stride < width", lambda: f(s=IMG - 1), INVALID, message, False)
        case(fn + ": width above the capacity", lambda: f(w=IMG + 1, s=IMG + 1), INVALID, message, False)

    # ---- single-sequence calls
    singles = [("vloam_scan_registration", True, scan1), ("vloam_scan_registration_device", False, scan1),
               ("vloam_process_scan", True, scan1), ("vloam_process_scan_device", False, scan1),
               ("vloam_process_frame", True, frame1), ("vloam_process_frame_device", False, frame1)]
    for fn, host, make in singles:
        f = make(fn, host)
        if B > 1:
            case(fn + ": two-session handle", f, INVALID, ONE_SEQ)
            continue
        case(fn + ": null handle", lambda f=f: f(hh=None), INVALID)
        case(fn + ": null cloud", lambda f=f: f(p=None), INVALID)
        case(fn + ": n == 0", lambda f=f: f(n=0), EMPTY_ST, EMPTY)
        case(fn + ": n == max_points + 1", lambda f=f: f(n=MP + 1), CAPACITY, TOO_BIG)
        if make is frame1:
            case(fn + ": n_match < 0", lambda f=f: f(pu=uv[0], cu=uv[0], m=-1), INVALID)
            case(fn + ": n_match > 0, null arrays", lambda f=f: f(m=5), INVALID)
            case(fn + ": n_match above kVoMaxMatches", lambda f=f: f(pu=uv[0], cu=uv[0], m=VO_MAX + 1), CAPACITY, TOO_MANY)
    for fn, host in (("vloam_process_frame_image", True), ("vloam_process_frame_image_device", False)):
        f = image1(fn, host)
        if B > 1:
            if with_image:
                case(fn + ": two-session handle", f, INVALID, ONE_SEQ)
            continue
        if not with_image:
            case(fn + ": no image front-end", f, ORDER, NO_IMG)
            continue
        case(fn + ": null handle", lambda f=f: f(hh=None), INVALID)
        case(fn + ": null cloud", lambda f=f: f(p=None), INVALID)
        case(fn + ": null image", lambda f=f: f(g=None), INVALID)
        case(fn + ": n == 0", lambda f=f: f(n=0), EMPTY_ST, EMPTY)
        case(fn + ": n == max_points + 1", lambda f=f: f(n=MP + 1), CAPACITY, TOO_BIG)
        image_size_cases(fn, f, HOST_IMG if host else DEV_IMG)
    # vloam_vo_process_point_cloud: its own statuses, no message (see the module's docstring)
    f = scan1("vloam_vo_process_point_cloud", True)
    if B > 1:
        case("vloam_vo_process_point_cloud: two-session handle", f, INVALID, ONE_SEQ)
    else:
        case("vloam_vo_process_point_cloud: null handle", lambda f=f: f(hh=None), INVALID)
        case("vloam_vo_process_point_cloud: null cloud", lambda f=f: f(p=None), INVALID)
        case("vloam_vo_process_point_cloud: n == 0", lambda f=f: f(n=0), INVALID)
        case("vloam_vo_process_point_cloud: n == max_points + 1", lambda f=f: f(n=MP + 1), CAPACITY)
    for fn, host in (("vloam_vo_process_image", True), ("vloam_vo_process_image_device", False)):
        f = voimg(fn, host)
        if not with_image:
            if B == 1:
                case(fn + ": no image front-end", f, ORDER, NO_IMG)
            continue
        if B > 1:
            case(fn + ": two-session handle", f, INVALID, ONE_SEQ)
            continue
        case(fn + ": null handle", lambda f=f: f(hh=None), INVALID)
        case(fn + ": null image", lambda f=f: f(g=None), INVALID)
        image_size_cases(fn, f, HOST_IMG if host else DEV_IMG)

    # ---- batch calls (session b = the last one holds the broken argument)
    for fn, host, make in (("vloam_batch_process_scan", True, scanB), ("vloam_batch_process_scan_device", False, scanB),
                           ("vloam_batch_process_frame", True, frameB), ("vloam_batch_process_frame_device", False, frameB)):
        f = make(fn, host)
        x = hx if host else dx
        case(fn + ": null handle", lambda f=f: f(hh=None), INVALID)
        case(fn + ": null cloud array", lambda f=f: f(null_p=True), INVALID)
        case(fn + ": null size array", lambda f=f: f(null_n=True), INVALID)
        case(fn + ": null cloud of a session", lambda f=f, x=x: f(p=swap(x, b, None)), INVALID, SENTINEL if host else null_sweep(b))
        case(fn + ": n == 0", lambda f=f: f(n=swap(n_ok, b, 0)), EMPTY_ST, EMPTY)
        case(fn + ": n == max_points + 1", lambda f=f: f(n=swap(n_ok, b, MP + 1)), CAPACITY, TOO_BIG)
        if make is frameB:
            case(fn + ": n_match < 0", lambda f=f: f(pu=uv, cu=uv, m=swap(zero, b, -1)), INVALID, bad_matches(b))
            case(fn + ": n_match > 0, null arrays", lambda f=f: f(m=swap(zero, b, 5)), INVALID, bad_matches(b))
            case(fn + ": n_match above kVoMaxMatches", lambda f=f: f(pu=uv, cu=uv, m=swap(zero, b, VO_MAX + 1)), CAPACITY, TOO_MANY)
    for fn, host in (("vloam_batch_process_frame_image", True), ("vloam_batch_process_frame_image_device", False)):
        f = imageB(fn, host)
        x, g = (hx if host else dx), (hg if host else dg)
        if not with_image:
            case(fn + ": no image front-end", f, ORDER, NO_IMG)
            continue
        case(fn + ": null handle", lambda f=f: f(hh=None), INVALID)
        case(fn + ": null cloud array", lambda f=f: f(null_p=True), INVALID)
        case(fn + ": null size array", lambda f=f: f(null_n=True), INVALID)
        case(fn + ": null image array", lambda f=f: f(null_g=True), INVALID)
        case(fn + ": null cloud of a session", lambda f=f, x=x: f(p=swap(x, b, None)), INVALID, SENTINEL if host else null_sweep(b))
        case(fn + ": null image of a session", lambda f=f, g=g: f(g=swap(g, b, None)), INVALID, SENTINEL if host else null_image(b))
        case(fn + ": n == 0", lambda f=f: f(n=swap(n_ok, b, 0)), EMPTY_ST, EMPTY)
        case(fn + ": n == max_points + 1", lambda f=f: f(n=swap(n_ok, b, MP + 1)), CAPACITY, TOO_BIG)
        image_size_cases(fn, f, HOST_IMG if host else DEV_IMG)
    return out


def run_refusals(vl, hd, cases):
    """Every case: the status, the message and the frame count, all mismatches reported together."""
    L = hd.L
    wrong = []
    for name, call, status, message, exact in cases:
        junk = C.c_void_p()
        assert L.vloam_create_batch(C.byref(hd.cfg), 0, 0, C.byref(junk)) == vl.ERR_INVALID and L.vloam_last_error() == SENTINEL
        before = hd.frame_count()
        st = call()
        err = L.vloam_last_error()
        if st != status:
            wrong.append("%s: status %d, expected %d (%r)" % (name, st, status, err))
        if (err != message) if exact else (not err.startswith(message)):
            wrong.append("%s: message %r, expected %r" % (name, err, message))
        if hd.frame_count() != before:
            wrong.append("%s: vloam_frame_count went from %d to %d" % (name, before, hd.frame_count()))
    return wrong


def three_sweeps(hd, inp):
    """Sweeps 0..2 (session 1: 3..5) through the host whole-sweep call; the trajectory rows of every session, as bytes."""
    L, B = hd.L, hd.n_sessions
    for k in range(3):
        if B == 1:
            st = L.vloam_process_scan(hd.h, C.c_void_p(inp.host[k].ctypes.data), MP)
        else:
            st = L.vloam_batch_process_scan(hd.h, vp(*[inp.host[k + 3 * s].ctypes.data for s in range(B)]), ci(*[MP] * B))
        assert st == 0, L.vloam_last_error()
    assert L.vloam_sync(hd.h) == 0, L.vloam_last_error()
    rows = []
    for s in range(B):
        assert L.vloam_select_session(hd.h, s) == 0
        t = np.zeros((3, 14))
        assert L.vloam_get_trajectory(hd.h, 0, 3, C.c_void_p(t.ctypes.data)) == 0, L.vloam_last_error()
        assert np.isfinite(t).all() and np.abs(t[2, 4:7]).max() > 0
        rows.append(t.tobytes())
    return rows


@pytest.mark.parametrize("B,with_image", [(1, False), (1, True), (2, False), (2, True)],
                         ids=["single", "single_image", "two_sessions", "two_sessions_image"])
def test_refusals_leave_the_handle_as_it_was(vl, synth, inputs, B, with_image):
    hd = make_handle(vl, synth, B, with_image, calibrated=False)
    wrong = run_refusals(vl, hd, refusal_cases(hd.L, hd.h, B, with_image, inputs, calibrated=False))
    calibrate(hd, synth)
    cases = refusal_cases(hd.L, hd.h, B, with_image, inputs, calibrated=True)
    assert len(cases) >= (20 if B == 1 else 30)
    wrong += run_refusals(vl, hd, cases)
    after = three_sweeps(hd, inputs)
    assert hd.frame_count() == 3
    hd.close()
    fresh = make_handle(vl, synth, B, with_image)
    expected = three_sweeps(fresh, inputs)
    fresh.close()
    assert not wrong, "\n".join(wrong)
    assert after == expected   # the same calls fed both runs: exact equality
