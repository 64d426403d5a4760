"""Every optional ``settings`` key this package adds to the reference's ``config.json`` (a reference file has none of them) in one table,
``KEYS`` -- default, validator, what the key does -- and the readers ``Scene`` delegates to.  Host only.  ``validate`` runs every validator of
the table before any GPU call.  Read besides these: the reference's own ``opt_sync`` (False freezes alpha / beta) and ``device``."""
from collections import namedtuple
from functools import partial

import numpy as np

from .. import _lib

FREEZE_NAMES = ('alpha', 'beta', 'rs', 'R', 't', 'K', 'd')


def as_dict(settings):
    """``Scene.settings`` as a dict: a Scene that was given none holds ``[]`` (the reference's initial value), which reads as no key set."""
    return settings if isinstance(settings, dict) else {}


def solver_and_jacobian(st):
    """(MVUS_SOLVER_*, MVUS_JAC_*) of settings['ba_solver'] / settings['ba_jacobian']."""
    name = st.get('ba_solver', 'trf')
    if name not in ('trf', 'lm'):
        raise ValueError("settings['ba_solver'] must be 'trf' or 'lm', not %r" % (name,))
    modes = {'analytic': _lib.JAC_ANALYTIC, 'pattern': _lib.JAC_PATTERN, 'fd': _lib.JAC_FD}
    jac = st.get('ba_jacobian', 'analytic' if name == 'lm' else 'fd')
    if jac not in modes:
        raise ValueError("settings['ba_jacobian'] must be one of %s, not %r" % (sorted(modes), jac))
    return (_lib.SOLVER_LM_SCHUR if name == 'lm' else _lib.SOLVER_TRF_LSMR), modes[jac]


def loss(st):
    """(MVUS_LOSS_* code, f_scale) of settings['ba_loss'] / settings['ba_f_scale']."""
    name = st.get('ba_loss', 'linear')
    if not isinstance(name, str) or name not in _lib.LOSS_NAMES:
        raise ValueError("settings['ba_loss'] must be one of %s, not %r" % (sorted(_lib.LOSS_NAMES), name))
    f_scale = st.get('ba_f_scale', 1.0)
    if isinstance(f_scale, bool) or not isinstance(f_scale, (int, float, np.integer, np.floating)) or not np.isfinite(f_scale) or not f_scale > 0:
        raise ValueError("settings['ba_f_scale'] must be a finite positive number, not %r" % (f_scale,))
    if name != 'linear':
        if st.get('ba_solver', 'trf') != 'lm':
            raise ValueError("settings['ba_loss'] = %r needs settings['ba_solver'] = 'lm' (the TRF + LSMR solver has no robust loss), not %r"
                             % (name, st.get('ba_solver', 'trf')))
        if st.get('ba_jacobian', 'analytic') != 'analytic':
            raise ValueError("settings['ba_loss'] = %r needs settings['ba_jacobian'] = 'analytic', not %r" % (name, st.get('ba_jacobian')))
    return _lib.LOSS_NAMES[name], float(f_scale)


def freeze(st):
    """({camera index: names}, gauge) of settings['ba_freeze'] / settings['ba_gauge']."""
    gauge = st.get('ba_gauge', 'free')
    if not isinstance(gauge, str) or gauge not in ('free', 'anchor'):
        raise ValueError("settings['ba_gauge'] must be 'free' or 'anchor', not %r" % (gauge,))
    raw = {} if st.get('ba_freeze') is None else st['ba_freeze']
    if not isinstance(raw, dict):
        raise ValueError("settings['ba_freeze'] must map camera indices to lists of names from %s, not %r" % (list(FREEZE_NAMES), raw))
    out = {}
    for key, names in raw.items():
        try:                                 # (a config.json has string keys)
            cam = int(key)
            if isinstance(key, (bool, float)) or str(cam) != str(key).strip() or cam < 0:
                raise ValueError
        except (TypeError, ValueError):
            raise ValueError("settings['ba_freeze']: %r is not a camera index" % (key,)) from None
        if isinstance(names, str) or not isinstance(names, (list, tuple, set, frozenset)):
            raise ValueError("settings['ba_freeze'][%r] must be a list of names from %s, not %r" % (key, list(FREEZE_NAMES), names))
        for name in names:
            if not isinstance(name, str) or name not in FREEZE_NAMES:
                raise ValueError("settings['ba_freeze'][%r]: unknown name %r (one of %s)" % (key, name, list(FREEZE_NAMES)))
            if name in ('K', 'd') and not st.get('opt_calib', False):
                raise ValueError("settings['ba_freeze'][%r]: %r is a parameter only with settings['opt_calib'] (fixed calibration is not in x)" % (key, name))
        out.setdefault(cam, set()).update(names)
    return out, gauge


def flag(st, key):
    """settings[key] as a bool (absent = False); anything but a bool raises."""
    v = st.get(key, False)
    if not isinstance(v, (bool, np.bool_)):
        raise ValueError("settings['%s'] must be true or false, not %r" % (key, v))
    return bool(v)


def needs_lm(st, key, what):
    """``flag(st, key)`` of a feature that only the LM solver has: switched on with another ``ba_solver`` it raises."""
    on = flag(st, key)
    if on and st.get('ba_solver', 'trf') != 'lm':
        raise ValueError("settings['%s'] needs settings['ba_solver'] = 'lm' (the TRF + LSMR solver takes no %s), not %r" % (key, what, st.get('ba_solver', 'trf')))
    return on


def register_beta_search(st):
    """settings['ba_register_beta_search']: absent / None -> None, else (half_width, step) in frames, finite, half_width >= 0, step > 0."""
    v = st.get('ba_register_beta_search', None)
    if v is None:
        return None
    ok = isinstance(v, (list, tuple)) and len(v) == 2 and all(
        not isinstance(q, (bool, np.bool_)) and isinstance(q, (int, float, np.integer, np.floating)) and np.isfinite(q) for q in v)
    if not ok or not (v[0] >= 0 and v[1] > 0):
        raise ValueError("settings['ba_register_beta_search'] must be [half_width, step] in frames (finite, half_width >= 0, step > 0), not %r" % (v,))
    return float(v[0]), float(v[1])


def solve_options(st, solver, jac_mode, max_iter):
    """The ``MvusSolveOpts`` of one ``Scene.BA``: the library's defaults with settings['ba_lambda_min'] / ['ba_trust_radius'] over them."""
    opts = _lib.default_opts(solver, jac_mode, max_iter)
    opts.lm_lambda_min = float(st.get('ba_lambda_min', opts.lm_lambda_min))
    opts.lm_trust_radius = float(st.get('ba_trust_radius', opts.lm_trust_radius))
    return opts


def traj_weights(st, num_cam):
    """settings['traj_weights'], ['traj_sigma_px'], ['traj_weight_floor']: None (absent) or (mode, sigma_px (num_cam,), floor).  Not in ``validate``."""
    mode = st.get('traj_weights')
    if mode is None:
        return None
    if mode != 'triangulation':
        raise ValueError("settings['traj_weights'] must be 'triangulation' or absent, not %r" % (mode,))
    px = np.asarray(st.get('traj_sigma_px', 1.0), dtype=np.float64)
    if px.ndim > 1 or (px.ndim == 1 and px.size != num_cam) or not np.all(np.isfinite(px)) or not np.all(px > 0):
        raise ValueError("settings['traj_sigma_px'] must be a positive number, or one per camera")
    floor = float(st.get('traj_weight_floor', 1e-3))
    if not (0.0 < floor <= 1.0):
        raise ValueError("settings['traj_weight_floor'] must lie in (0, 1]")
    return mode, np.broadcast_to(px, (num_cam,)), floor


def _by(reader):                             # a reader of several keys as the validator of one of them
    return lambda st, key: reader(st)


# default: None where it depends on another key or is the library's.  check(st, key) raises ValueError on a bad value; None marks a key
# that is deliberately NOT validated (read as it is where it is used).  The order of the rows is the order in which bad keys are reported.
Key = namedtuple('Key', 'default check doc')
KEYS = {
    'ba_solver': Key('trf', _by(solver_and_jacobian), """'trf' = scipy's TRF + LSMR restated on the GPU -- with ``ba_jacobian`` 'fd' (its default) this
        is the reference's algorithm end to end: same pattern matrix, same grouped 2-point differences, same trust region, same termination;
        results agree with the reference's within the reference's own reproducibility.  'lm' = Levenberg-Marquardt on device-assembled normal
        equations with the Schur complement and the analytic Jacobian: ~20x faster per BA iteration, reaches a LOWER value of the same objective,
        hence another point than the reference's (DESIGN.md section 2 states how far, against the reference and against ground truth)."""),
    'ba_jacobian': Key(None, _by(solver_and_jacobian), """'fd' (default with 'trf'), 'pattern' = analytic, masked to the reference sparsity pattern,
        'analytic' = full analytic (default with 'lm')."""),
    'ba_pattern_ties': Key('numpy', None, """'numpy' = the twin rows of the pattern decided like np.argsort of this process decides them (what the
        reference would build here), 'canonical'."""),
    'ba_lambda_min': Key(None, None, """floor of the LM damping (default 3e-3, see ``mvus_solve_opts.lm_lambda_min``; the incremental loop of
        ``mvus_amd.pipeline`` sets 0.3 for its staged BAs unless told otherwise: ``common.LOOP_LM_LAMBDA_MIN``)."""),
    'ba_trust_radius': Key(None, None, """with 'lm': scipy's trust region on the length of the step, 0 = start from the norm of x0 (default: off, see
        ``mvus_solve_opts.lm_trust_radius``)."""),
    'ba_lm_wide_band': Key('trf', None, """with 'lm': what to do when the motion rows reach over more than six control points (knots less than a
        frame apart, i.e. more control points than detections): 'trf' solves THAT problem with TRF + LSMR on the analytic Jacobian and says so,
        'lm' keeps LM + Schur (general band solver, damping floor 0.3)."""),
    'ba_loss': Key('linear', _by(loss), """with 'lm': the ``loss`` ('linear', 'soft_l1', 'huber', 'cauchy', 'arctan') and, as ``ba_f_scale``, the
        ``f_scale`` (pixels) arguments of scipy's least_squares, which the reference never passes: gross outliers stop pulling on the first BA,
        the one that runs before ``remove_outliers`` can cut them.  Not with 'trf' (ValueError), and a problem the wide-band policy above would
        hand to TRF raises instead of dropping the loss."""),
    'ba_f_scale': Key(1.0, _by(loss), """see ``ba_loss``."""),
    'ba_gauge': Key('free', _by(freeze), """'free' (the reference's problem, similarity gauge left to the solver) or 'anchor' (``Scene.ba_frozen_mask``):
        the pose of ``sequence[0]`` and one translation component of ``sequence[1]`` are held -- the seven degrees of freedom of the similarity, no more."""),
    'ba_freeze': Key({}, _by(freeze), """{camera index: [names]} with names from 'alpha', 'beta', 'rs', 'R', 't', 'K', 'd': those parameters of that
        camera are held constant during BA (``mvus_ba_set_frozen``; both solvers).  'K' and 'd' need ``opt_calib`` (they are not parameters
        otherwise); cameras outside the BA's ``sequence[:numCam]`` are ignored for that BA.  The reference can only switch a group off for every
        camera at once (``opt_sync``, ``rs``, ``opt_calib``)."""),
    'ba_covariance': Key(False, flag, """True: ``mvus_amd.pipeline.reconstruct_from_config`` calls ``Scene.ba_covariance`` after the last BA and the
        output pickle carries its dict (``Scene.covariance``).  Needs a fixed gauge (``ba_gauge: 'anchor'`` or ``ba_freeze``)."""),
    'ba_kinematics': Key(False, flag, """True: ``reconstruct_from_config`` calls ``Scene.kinematics`` after ``spline_to_traj`` (after
        ``Scene.ba_covariance``, with its band, when ``ba_covariance`` is on too) and the output pickle carries its dict."""),
    'ba_detection_covariance': Key(False, flag, """True: ``reconstruct_from_config`` calls ``Scene.ba_detection_covariance`` after the last BA (one call
        that also yields ``Scene.covariance`` when ``ba_covariance`` is on) and the output pickle carries its dict (``Scene.detection_covariance``):
        per detection the signed residual, the 1-sigma ellipse of the fitted detection and the studentised residual."""),
    'ba_register': Key(False, flag, """True: the incremental loop of ``mvus_amd.pipeline`` calls ``Scene.register_camera`` on every new camera between
        ``get_camera_pose`` and ``triangulate``: alpha, beta, rs and the pose of THAT camera are adjusted against the trajectory as it stands
        (``mvus_ba_register_cameras``: Levenberg-Marquardt per camera on the device), the spline and the other cameras untouched."""),
    'ba_register_beta_search': Key(None, _by(register_beta_search), """[half_width, step] (frames): ``register_camera`` starts from beta + k step,
        |k step| <= half_width, all in one call, and keeps the start with the most inliers."""),
    'ba_position_priors': Key(False, partial(needs_lm, what='position priors'), """True with 'lm': ``Scene.position_priors`` -- surveyed positions (a
        GPS / RTK log) as a (7, K) array of t, x, y, z, sigma_x, sigma_y, sigma_z on the spline's timeline -- enter ``Scene.BA`` as observations
        (``mvus_ba_set_position_priors``): three non-collinear ones fix the similarity gauge, and the trajectory, the poses and their covariance
        come out in the surveyed frame, in its unit.  ``reconstruct_from_config`` then runs its loop as always, aligns the scene to the priors
        (``Scene.align_to_position_priors``) and ends with one LM BA over all cameras that carries them.  Not with 'trf' (ValueError), and a
        problem the wide-band policy above would hand to TRF raises instead of dropping the priors."""),
    'ba_landmarks': Key(False, partial(needs_lm, what='landmarks'), """True with 'lm': ``Scene.landmarks`` (3, L) -- surveyed static points -- and
        ``Scene.landmark_observations`` (6, K): camera id, landmark, u, v, sigma_u, sigma_v -- enter ``Scene.BA`` as observations
        (``mvus_ba_set_landmarks``): two rows per click that involve the clicked camera only and fix the similarity gauge, scale included.
        ``reconstruct_from_config`` runs the incremental loop as without them, then moves the result into the surveyed frame
        (``Scene.align_to_landmarks``) and ends with one LM BA over all cameras that carries them.  Not with 'trf' (ValueError); a problem the
        wide-band policy above would hand to TRF raises; ``register_camera`` raises while the setting is on and the scene holds landmarks."""),
    'ba_deterministic': Key(None, None, """accepted and ignored: the 'lm' solver's normal equations are assembled without floating-point atomics
        (one writer, one order of additions per entry) -- the same bits on every run by construction."""),
}


def validate(st):
    """Every validated key of ``KEYS`` checked, in table order (the arrays of priors and landmarks live on the Scene: ``Scene.ba_mode`` checks them)."""
    for name, key in KEYS.items():
        if key.check is not None:
            key.check(st, name)


