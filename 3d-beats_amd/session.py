"""A whole frame of the reference's app, from the camera's depth frame to note events: `App_3d_bz.tick` and
`run_per_hand_pipeline` (src/3d_bz.py:133-286, 388-522 of the reference) without camera, GUI or MIDI.

`BeatsSession` owns a `FrameFrontEnd` (raw depth -> table-free depth), a `HandGrouping` (-> the hand-group image), two
`HandPipeline`s (right hand: group 1, unflipped; left hand: group 2, flipped; the second on a sibling of the forest stack)
and ONE `HandState` of ten fingertips (right 0-4, left 5-9).  Everything runs on the current stream; a frame is enqueued by
`tick()` and nothing is read until `poll()`.  The fingertip heights are looked up in the raw camera frame, as the reference
does (3d_bz.py:517), and the heights read the front end's plane on the device, so a recalibration reaches them.

With `post_filter=` (a `DepthPostFilter`) every raw frame goes through the depth post-filter first, and "the raw frame" above
is the filtered one: the front end, both hands and the fingertip heights see it.
"""
import numpy as np

from . import _lib
from .device import DeviceArray, get_runtime
from .frontend import FrameFrontEnd
from .grouping import HandGrouping
from .hand_state import MAX_VELOCITY, MIN_VELOCITY, VELOCITY_SENSITIVE, HandState
from .pipeline import DEFAULT_TIP_MAX_DIST, DEFAULT_TIP_Z_TOL, HandPipeline

TRAIN_DIM_X = 848


class _Frame:
    """One frame of a batch buffer behind the `.cu()` that HandPipeline asks of its images."""

    def __init__(self, array):
        self._cu, self.shape, self.dtype = array, array.shape, array.dtype

    def cu(self):
        return self._cu


class BeatsSession:
    def __init__(self, layered_rdf, depth_dims, intrinsics, on_fn=None, off_fn=None, labels_reduce=2, depth_mm_level=3,
                 group_min_size=0.06, plane_z_threshold=40., gauss_sigma=2.0, mean_shift_rounds=6,
                 mean_shift_variances=(50., 8., 8., 8., 8., 8., 8.), fingertip_idxes=(2, 3, 4, 5, 6), z_thresh_offset=25.,
                 min_velocity=10., max_velocity=120., velocity_sensitive=True, scale_factor=None,
                 fingertip_thresholds=(200., 160., 160., 160., 160.), first_notes=(36, 41), max_frames=8,
                 num_random_guesses=25000, seed=None, fused_io=True, capacity=4096, post_filter=None, soft_modes=False,
                 joint_votes=None, tip_joints=None, tip_policy='fill', tip_max_dist=DEFAULT_TIP_MAX_DIST,
                 tip_z_tol=DEFAULT_TIP_Z_TOL, shapes=None, on_shape_fn=None):
        """layered_rdf: a LayeredDecisionForest built for depth_dims = (DIM_Y, DIM_X) and labels_reduce; intrinsics = (focal,
        ppx, ppy) of the depth camera.  The other defaults are the app's (3d_bz.py:49-124); scale_factor = DIM_X / 848 when
        None.  max_frames = the batch of run_sequence's front end and grouping.  post_filter: a DepthPostFilter of the same
        depth_dims that calibrate, tick and run_sequence pass their frames through first; its temporal state runs on from
        call to call (post_filter.reset() starts it afresh).  Without one nothing is allocated or launched for it.
        soft_modes: both hands' pipelines find their modes weighted by the stack's confidence (HandPipeline's soft_modes: needs
        fused_io and a layered_rdf with min_conf set); False, the default, changes nothing.
        joint_votes: (forest, table) or (forest, table, settings) -- a DecisionForest, a VoteTable fitted to it and a dict of
        JointVoter's keyword arguments (labels_reduce, cell_shift, box, min_support).  One JointVoter per hand is built for
        depth_dims with max_frames the session's and handed to the hand's pipeline with tip_joints, tip_policy, tip_max_dist
        and tip_z_tol (HandPipeline's; the left hand's frame is mirrored, so both hands use the same joints): tick and both
        kinds of run_sequence then step the notes from the voted fingertips' heights.  None, the default, changes nothing.
        shapes: (forest,) or (forest, settings) -- a shape forest (hand_scene.make_shape_dataset, train_forest) and a dict of
        ShapeVoter's keyword arguments (labels_reduce, min_pixels, min_conf, hold, release, names).  One ShapeVoter per hand is
        built for depth_dims with max_frames the session's and handed to the hand's pipeline: tick and both kinds of
        run_sequence classify every frame of each hand, and the held shapes live on the device from call to call.
        on_shape_fn(hand, held): called by poll() -- hand 0 is the right hand, 1 the left -- see poll.  None, the default,
        changes nothing."""
        if shapes is not None:        # (refused before anything is allocated)
            from .shape import SETTINGS, ShapeVoter
            if not isinstance(shapes, (tuple, list)) or not 1 <= len(shapes) <= 2:
                raise ValueError("shapes is (forest,) or (forest, settings)")
            shape_settings = dict(shapes[1]) if len(shapes) == 2 else {}
            if "max_frames" in shape_settings:
                raise ValueError("shapes: the voters' max_frames is the session's")
            if set(shape_settings) - set(SETTINGS):
                raise ValueError(f"shapes: unknown settings {sorted(set(shape_settings) - set(SETTINGS))}")
            if not fused_io:
                raise ValueError("shapes needs fused_io=True")
        self._rt = get_runtime()
        self.DIM_Y, self.DIM_X = int(depth_dims[0]), int(depth_dims[1])
        self.max_frames = int(max_frames)
        focal, ppx, ppy = (float(v) for v in intrinsics)
        scale = self.DIM_X / TRAIN_DIM_X if scale_factor is None else float(scale_factor)
        n = len(fingertip_idxes)
        assert len(fingertip_thresholds) == n
        self.front_end = FrameFrontEnd((self.DIM_Y, self.DIM_X), (focal, ppx, ppy), plane_z_threshold, gauss_sigma=gauss_sigma,
                                       num_random_guesses=num_random_guesses, seed=seed)
        self.grouping = HandGrouping((self.DIM_Y, self.DIM_X), depth_mm_level, group_min_size, max_frames=self.max_frames)
        defaults = [(fingertip_thresholds[i], first + i) for first in first_notes for i in range(n)]
        self.hand_state = HandState(defaults, on_fn, off_fn, capacity=capacity)
        self.hand_state.set_field(MIN_VELOCITY, [min_velocity] * (2 * n))
        self.hand_state.set_field(MAX_VELOCITY, [max_velocity] * (2 * n))
        self.hand_state.set_field(VELOCITY_SENSITIVE, [1. if velocity_sensitive else 0.] * (2 * n))
        self.hand_state.z_thresh_offset = z_thresh_offset
        args = ((self.DIM_Y, self.DIM_X), labels_reduce, scale, mean_shift_rounds, list(mean_shift_variances),
                list(fingertip_idxes), (focal, focal, ppx, ppy), self.front_end.calibrated_plane.plane_cu)
        voters, tips = (None, None), {}
        if joint_votes is not None:
            from .joint_votes import JointVoter
            if not 2 <= len(joint_votes) <= 3:
                raise ValueError("joint_votes is (forest, table) or (forest, table, settings)")
            settings = dict(joint_votes[2]) if len(joint_votes) == 3 else {}
            if "max_frames" in settings:
                raise ValueError("joint_votes: the voters' max_frames is the session's")
            voters = tuple(JointVoter(joint_votes[0], joint_votes[1], (self.DIM_Y, self.DIM_X), max_frames=self.max_frames,
                                      **settings) for _ in range(2))
            tips = dict(tip_joints=tip_joints, tip_policy=tip_policy, tip_max_dist=tip_max_dist, tip_z_tol=tip_z_tol)
        shape_voters = (None, None)
        if shapes is not None:
            shape_voters = tuple(ShapeVoter(shapes[0], (self.DIM_Y, self.DIM_X), max_frames=self.max_frames, **shape_settings)
                                 for _ in range(2))
        self.on_shape_fn, self.last_shapes, self._delivered_shapes = on_shape_fn, None, [-1, -1]
        self.right = HandPipeline(layered_rdf, *args, depth_mm_level=depth_mm_level, fused_io=fused_io,
                                  hand_state=self.hand_state, tip_first=0, soft_modes=soft_modes, joint_voter=voters[0],
                                  shape_voter=shape_voters[0], **tips)
        self.left = HandPipeline(layered_rdf, *args, depth_mm_level=depth_mm_level, fused_io=fused_io,
                                 hand_state=self.hand_state, tip_first=n, soft_modes=soft_modes, joint_voter=voters[1],
                                 shape_voter=shape_voters[1], **tips)
        self.n_tips = 2 * n
        hm, wm = self.grouping.depth_mm_dims
        self._raw = DeviceArray((self.max_frames, self.DIM_Y, self.DIM_X), np.uint16)
        self._clean = DeviceArray((self.max_frames, self.DIM_Y, self.DIM_X), np.uint16)
        self.post_filter = post_filter
        if post_filter is not None:
            assert (post_filter.DIM_Y, post_filter.DIM_X) == (self.DIM_Y, self.DIM_X), "post_filter is of another frame size"
            self._filtered = DeviceArray((self.max_frames, self.DIM_Y, self.DIM_X), np.uint16)
        self._groups = DeviceArray((self.max_frames, hm, wm), np.uint16)
        self._clean_f = [_Frame(self._clean[i]) for i in range(self.max_frames)]
        self._groups_f = [_Frame(self._groups[i]) for i in range(self.max_frames)]

    # -- the plane --
    def calibrate(self, depth):
        """Fit the table plane to a frame (host or device uint16 [DIM_Y, DIM_X]); returns the 4x4 plane."""
        return self.front_end.calibrate(self._camera_frames(depth, 1)[0])

    def set_plane(self, plane):
        self.front_end.set_plane(plane)

    def _on_device(self, frames, n):
        """uint16 [n, DIM_Y, DIM_X] on the device: the frames themselves, or their copy in this session's raw buffer."""
        if hasattr(frames, "cu"):
            frames = frames.cu()
        if isinstance(frames, DeviceArray):
            return frames.reshape((n, self.DIM_Y, self.DIM_X))
        self._raw[:n].set(np.ascontiguousarray(frames, np.uint16).reshape(n, self.DIM_Y, self.DIM_X))
        return self._raw[:n]

    def _camera_frames(self, frames, n):
        """_on_device, then the post-filter when there is one: what the rest of the frame takes for the camera's frames."""
        raw = self._on_device(frames, n)
        if self.post_filter is None:
            return raw
        return self.post_filter.run(raw, self._filtered[:n])

    # -- live --
    def tick(self, depth):
        """Enqueues one whole frame (uint16 [DIM_Y, DIM_X]) on the current stream and returns nothing: front end, grouping,
        both hands, the note step.  A device frame is only enqueued and the stream is never waited for; a host frame is
        copied to the device first."""
        raw = self._camera_frames(depth, 1)
        self.front_end.run(raw, self._clean[:1])
        self.grouping.make_group_image(self._clean[:1], self._groups[:1])
        raw = _Frame(raw[0])
        # the right hand's launch precedes the left's: events of a frame come out right hand first
        self.right.enqueue(self._clean_f[0], self._groups_f[0], 1, False, height_depth=raw)
        self.left.enqueue(self._clean_f[0], self._groups_f[0], 2, True, height_depth=raw)

    def poll(self):
        """HandState.poll(): waits for the stream and delivers the events since the last poll.  With `shapes` and an
        on_shape_fn it then reads each hand's held shape (16 bytes a hand) and calls on_shape_fn(hand, held) for a hand whose
        held shape differs from the one last delivered (-1, no shape, at the start).  Only the latest state is delivered:
        changes between two polls collapse -- a shape that came and went between them is never seen, and one that changed
        twice arrives as one call.  The per-frame rows are in `last_shapes` after run_sequence."""
        events = self.hand_state.poll()
        if getattr(self, "on_shape_fn", None) is not None and getattr(self.right, "shape_voter", None) is not None:
            for hand, pipe in enumerate((self.right, self.left)):
                held = int(pipe.shape_voter.state.get()[0])
                if held != self._delivered_shapes[hand]:
                    self._delivered_shapes[hand] = held
                    self.on_shape_fn(hand, held)
        return events

    # -- offline --
    def run_sequence(self, frames, batched=False):
        """frames: uint16 [F, DIM_Y, DIM_X] on the host or the device.  The front end and the grouping run in batches of
        max_frames; one synchronisation, at the end.  Returns (events, heights float64 [F, 10]).  The heights log is
        written on the device and read once, after the last frame.
        batched=False: the per-hand chains run frame by frame; each hand's heights are copied into the frame's row behind
        its chain (a stream-ordered copy of 40 bytes).
        batched=True (needs fused_io): the per-hand chains take the whole block too -- HandPipeline.enqueue_batch for the
        right hand writes columns 0-4 of the block's log rows, for the left hand columns 5-9, and ONE note step advances
        all ten fingertips over the block's frames.  Same events, heights and state, bit for bit; a prepare, one launch a
        forest layer, a composite and a mean shift per hand and block instead of per hand and frame, and no copies.
        With `shapes` the rows (raw, conf, held, changed) of every frame and hand are logged on the device too and left in
        `last_shapes`, host int32 [F, 2, 4] (right hand first), read once after the last frame: the same bytes for both
        kinds of run, and the voters' state runs on from call to call."""
        if batched and not (self.right.fused_io and self.left.fused_io):
            raise ValueError("run_sequence(batched=True) needs a session built with fused_io=True")
        F = int(frames.shape[0])
        n = self.n_tips // 2
        log = DeviceArray((max(F, 1), self.n_tips), np.float64)
        lib, stream = self._rt.lib, self._rt.stream
        shape_log = DeviceArray((2, max(F, 1), 4), np.int32) if getattr(self.right, "shape_voter", None) is not None else None

        def log_shapes(hand, rows, first, count):
            rc = lib.rdf_memcpy_device_async(shape_log.ptr + (hand * max(F, 1) + first) * 16, rows.ptr, count * 16, stream())
            _lib.check(lib, rc, "rdf_memcpy_device_async")
        for a in range(0, F, self.max_frames):
            b = min(F - a, self.max_frames)
            raw = self._camera_frames(frames[a:a + b], b)
            self.front_end.run(raw, self._clean[:b])
            self.grouping.make_group_image(self._clean[:b], self._groups[:b])
            if batched:
                row = log.ptr + a * self.n_tips * 8
                # the right hand's columns precede the left's: events of a frame come out right hand first, as in tick()
                self.right.enqueue_batch(self._clean[:b], self._groups[:b], 1, False, raw, row, self.n_tips)
                self.left.enqueue_batch(self._clean[:b], self._groups[:b], 2, True, raw, row + n * 8, self.n_tips)
                self.hand_state.step_device(row, 0, self.n_tips, n_frames=b)
                if shape_log is not None:
                    log_shapes(0, self.right.shape_batch, a, b)
                    log_shapes(1, self.left.shape_batch, a, b)
                continue
            for i in range(b):
                raw_i = _Frame(raw[i])
                for pipe in (self.right, self.left):
                    g_id, flip = (1, False) if pipe is self.right else (2, True)
                    pipe.enqueue(self._clean_f[i], self._groups_f[i], g_id, flip, height_depth=raw_i)
                    rc = lib.rdf_memcpy_device_async(log.ptr + ((a + i) * self.n_tips + pipe.tip_first) * 8, pipe.heights_ptr,
                                                     n * 8, stream())
                    _lib.check(lib, rc, "rdf_memcpy_device_async")
                    if shape_log is not None:
                        log_shapes(0 if pipe is self.right else 1, pipe.shape, a + i, 1)
        events = self.poll()
        if shape_log is not None:
            self.last_shapes = np.ascontiguousarray(shape_log.get()[:, :F].transpose(1, 0, 2))
        return events, log.get()[:F]
