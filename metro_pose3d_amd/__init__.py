"""metro_pose3d_amd: MI355X (gfx950) implementation of the MeTRo inference hot path.

Public surface (mirrors reference inference.py):
    estimate_pose(images, model_path) -> (poses, joint_edges, joint_names)
        [, PoseUncertainty with return_uncertainty=True][, Heatmaps (per-joint xy and z marginals) with return_heatmaps=True]
    estimate_pose_modes(images, model_path, k=2, radius=1) -> the same, and Modes last: the k places each joint may be, with the
        probability mass, position (mm) and covariance of each
    estimate_pose_posterior(images, model_path, prior_positions, prior_precision) -> the same, and Posterior last: each joint's
        heat-map times a Gaussian prior (pose_prior: mm -> prior rows) -- posterior position, covariance and log-evidence
    estimate_pose_in_frames(frames, boxes, model_path, cameras=...) -> the same from uint8 frames + person boxes (frames.py)
    locate_poses_in_frames(frames, boxes, model_path, cameras=..., bone_lengths=...) -> absolute poses + 2D frame keypoints
    triangulate_poses_in_frames(frames, boxes, model_path, cameras, person_index, frame_index) -> world poses of persons seen
        by several calibrated cameras
    match_poses_in_frames(frames, boxes, model_path, cameras, frame_index) -> the same without a person_index: the boxes of
        the cameras are matched on the device by how close their rays pass
    track_poses_in_frames(frames, boxes, model_path, cameras, track_index, frame_index, timestamps) -> poses of tracked
        persons smoothed over the frames of a video (Kalman filter / RTS smoother weighted by the heat-map covariances)
    follow_poses_in_frames(frames, boxes, model_path, cameras, frame_index, timestamps) -> the same without a track_index:
        the boxes are assigned to tracks on the device, frame by frame, under ids that persist from call to call
    follow_world_poses_in_frames(frames, boxes, model_path, cameras, frame_index, timestamps) -> a calibrated rig's video:
        boxes matched across cameras per exposure, triangulated with covariance, followed and smoothed in the world
    follow_rig_poses_in_frames(frames, boxes, model_path, cameras, frame_index, timestamps) -> the same, and a person only
        one camera sees keeps feeding its track: its rays are matched to the tracks and update them across the ray
    predict_boxes_in_frames(tracks, cameras, frame_sizes, timestamps) -> the person boxes of the next frames from the
        table of tracks those two return (frame_sizes(frames): their sizes), for the frames a detector does not see
    locate_tracked_poses_in_frames(frames, boxes, model_path, cameras, tracks, track_index, frame_index, timestamps) ->
        locate_poses_in_frames with each person's own track as the prior of each crop's heat-maps: the plain poses, the
        posterior poses and covariance, and per joint the log-evidence a tracker gates with (Follower.locate)
    estimate_pose_skeleton(images, model_path, bone_lengths, k=2, radius=1) -> estimate_pose_modes and, last, SkeletonModes:
        which mode every joint is in under the person's bone lengths (exact inference on the skeleton tree), the marginals,
        the evidence; locate_skeleton_poses_in_frames(frames, boxes, model_path, cameras, bone_lengths, frame_index) -> the
        same choice in locate_poses_in_frames' chain (SkeletonFramePoses: plain bit for bit, and the selected poses beside it)
    fuse_poses_in_frames(frames, boxes, model_path, cameras, person_index, frame_index) -> triangulate_poses_in_frames
        and, beside it, every person's heat-maps fused over its cameras on a grid of world points: a wrong peak in one
        camera finds no partner in the others (FusedPoses: the triangulation bit for bit, the fused poses, covariance, ...)
    Follower(model_path, cameras, world=False, assignment='greedy', ...) -> one of the two follow calls with its keywords
        and its table of tracks kept from call to call: .follow(frames, boxes, frame_index, timestamps), .predict(...),
        .locate(frames, boxes, track_index, frame_index, timestamps);
        with world=True, learn_bones=True it also learns every followed person's bone lengths on the device, and
        .bone_lengths_for(track_index, fallback) hands them to locate_poses_in_frames(bone_lengths=...) as a CUDA tensor
plus the pieces under it: ModelSpec, Engine (plan + forward over libmetro_hip.so), the model
container (save_model / load_model) and batch sharding over the GPUs of a node (dist).
"""
from metro_pose3d_amd.spec import ModelSpec  # noqa: F401
from metro_pose3d_amd.modelfile import load_model, save_model  # noqa: F401

__all__ = ['ModelSpec', 'load_model', 'save_model', 'Engine', 'estimate_pose', 'Heatmaps', 'estimate_pose_modes', 'Modes', 'estimate_pose_skeleton', 'SkeletonModes', 'estimate_pose_posterior', 'Posterior', 'pose_prior', 'posterior_to_metric', 'estimate_pose_in_frames', 'locate_poses_in_frames', 'triangulate_poses_in_frames', 'match_poses_in_frames', 'track_poses_in_frames', 'follow_poses_in_frames', 'follow_world_poses_in_frames', 'follow_rig_poses_in_frames', 'predict_boxes_in_frames', 'locate_tracked_poses_in_frames', 'locate_skeleton_poses_in_frames', 'SkeletonFramePoses', 'fuse_poses_in_frames', 'FusedPoses', 'frame_sizes', 'Follower', 'Camera']


def __getattr__(name):
    # Engine / estimate_pose import torch; keep `import metro_pose3d_amd` light.
    if name == 'Engine':
        from metro_pose3d_amd.engine import Engine
        return Engine
    if name == 'estimate_pose':
        from metro_pose3d_amd.inference import estimate_pose
        return estimate_pose
    if name == 'Heatmaps':
        from metro_pose3d_amd.inference import Heatmaps
        return Heatmaps
    if name in ('estimate_pose_modes', 'Modes', 'estimate_pose_skeleton', 'SkeletonModes', 'estimate_pose_posterior', 'Posterior', 'pose_prior', 'posterior_to_metric'):
        from metro_pose3d_amd import inference
        return getattr(inference, name)
    if name in ('estimate_pose_in_frames', 'locate_poses_in_frames', 'triangulate_poses_in_frames', 'match_poses_in_frames', 'track_poses_in_frames', 'follow_poses_in_frames', 'follow_world_poses_in_frames', 'follow_rig_poses_in_frames', 'predict_boxes_in_frames', 'locate_tracked_poses_in_frames', 'locate_skeleton_poses_in_frames', 'SkeletonFramePoses', 'fuse_poses_in_frames', 'FusedPoses', 'frame_sizes', 'Follower', 'Camera'):
        from metro_pose3d_amd import frames
        return getattr(frames, name)
    raise AttributeError(name)
