"""Device-side face crop / inverse paste for the sampler's un-aligned prior branch.

Mirror of the two methods of the reference's ``FaceRestoreHelper`` that the sampling loop calls every denoising step
(``guided_diffusion/facelib/utils/face_restoration_helper.py:225-254`` ``get_crop_face_from_affine_matrices`` and
``:264-335`` ``inverse_faces``, called at ``gaussian_diffusion.py:476-493``), same names, argument meaning and return
values -- but the frames stay in HBM: the reference converts every frame to numpy, runs ``cv2.warpAffine`` /
``cv2.GaussianBlur`` on the host and uploads the result, twice per step.

The affine matrices are an INPUT: the reference estimates them once per window (``scripts/video_sample.py:446-448``,
RetinaFace landmarks + ``cv2.estimateAffinePartial2D``); that detector is not part of this package (network weights
and cv2 unavailable), so ``get_crop_face`` delegates to a ``detector`` object when one is supplied (e.g. the reference's
own helper) and raises otherwise.

OpenCV's arithmetic is restated from its published algorithm (opencv 4.4: fixed-point source coordinates, a = -0.75
cubic weight table, constant-border rule, separable float64 Gaussian with reflect-101): **parity unpinned** -- cv2 is not
installable in the build container and the reference holds no fixture of these calls.
"""
import numpy as np
import torch

from .. import ops

# facelib/utils/face_restoration_helper.py:283-303, written for ParseNet's label order (the only parser the reference pairs it
# with).  It is the default for BiSeNet too: parsing_bisenet.pth's label order cannot be inspected offline, so that pairing is
# PARITY UNPINNED; FaceRestoreHelper(mask_colormap=...) replaces the list.
MASK_COLORMAP = [0, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 0, 0, 0, 0, 0]


def invert_affine(M):
    """``cv2.invertAffineTransform`` (imgwarp.cpp), in double on the host: six numbers per face."""
    M = np.asarray(M, dtype=np.float64)
    D = M[0, 0] * M[1, 1] - M[0, 1] * M[1, 0]
    D = 1.0 / D if D != 0 else 0.0
    A11, A22, A12, A21 = M[1, 1] * D, M[0, 0] * D, -M[0, 1] * D, -M[1, 0] * D
    return np.array([[A11, A12, -A11 * M[0, 2] - A12 * M[1, 2]],
                     [A21, A22, -A21 * M[0, 2] - A22 * M[1, 2]]], dtype=np.float64)


def gaussian_kernel(ksize, sigma):
    """``cv2.getGaussianKernel(ksize, sigma, CV_64F)``."""
    x = np.arange(ksize, dtype=np.float64) - (ksize - 1) * 0.5
    k = np.exp((-0.5 / (sigma * sigma)) * x * x)
    return k * (1.0 / k.sum())


class FaceRestoreHelper(object):
    """``FaceRestoreHelper(face_size=512, device=..., face_parse=ParseNet)``: the crop / paste half of the reference class."""

    def __init__(self, face_size=512, crop_ratio=(1, 1), det_model="retinaface_resnet50", save_ext="png",
                 template_3points=False, device=None, face_parse=None, detector=None, face_det=None, mask_colormap=None):
        assert crop_ratio[0] >= 1 and crop_ratio[1] >= 1, "crop ration only supports >=1"
        self.face_size = (int(face_size * crop_ratio[1]), int(face_size * crop_ratio[0]))    # (w, h), as the reference
        self.device = torch.device(device if device is not None else "cuda")
        self.face_parse = face_parse          # a parser with parse_indices(x): parsenet.ParseNet or bisenet.BiSeNet (inverse_faces)
        # paste-mask value per parsing class (None: the reference's 19-entry list)
        self.mask_colormap = [float(v) for v in (MASK_COLORMAP if mask_colormap is None else mask_colormap)]
        self.detector = detector              # optional external object with a get_crop_face method (e.g. the reference's helper)
        self.face_det = face_det              # retinaface.RetinaFace (built on first use when None) or a loaded yolov5face.YoloDetector
        self.det_model = det_model
        self.template_3points = template_3points
        self.crop_ratio = crop_ratio
        if template_3points:
            self.face_template = np.array([[192, 240], [319, 240], [257, 371]], dtype=np.float64)
        else:                                 # standard 5 landmarks for FFHQ faces with 512 x 512 (face_restoration_helper.py:90-98)
            self.face_template = np.array([[192.98138, 239.94708], [318.90277, 240.1936], [256.63416, 314.01935],
                                           [201.26117, 371.41043], [313.08905, 371.15118]])
        self.face_template = self.face_template * (face_size / 512.0)
        if crop_ratio[0] > 1:
            self.face_template[:, 1] += face_size * (crop_ratio[0] - 1) / 2
        if crop_ratio[1] > 1:
            self.face_template[:, 0] += face_size * (crop_ratio[1] - 1) / 2
        self._const = {}
        self._minv_cache = {}
        self._index_cache = {}

    # -- detection half (facelib/utils/face_restoration_helper.py:122-224): RetinaFace on the HIP kernels, landmark alignment on
    # the host (five points per face), the crop itself by flair_warp_affine_cubic
    def _detector(self):
        if self.face_det is None:
            if "retinaface" not in self.det_model:
                raise NotImplementedError(f"flair_amd: det_model={self.det_model!r} is not built by the helper (it never runs a "
                                          "random-weight YOLOv5-face): pass a loaded yolov5face.YoloDetector as face_det=")
            from .retinaface import RetinaFace
            # random initialisation: load detection_Resnet50_Final.pth with face_det.load_state_dict(torch.load(path,
            # weights_only=True)) -- the reference downloads it at construction (facelib/detection/__init__.py:25-48)
            self.face_det = RetinaFace(network_name=self.det_model.split("_", 1)[1], half=False, device=self.device)
        return self.face_det

    def get_crop_face(self, bathed_imgs, only_keep_largest=False, only_center_face=False, resize=None, eye_dist_threshold=None,
                      face_template_resize=None, face_template_x_offset=None, face_template_y_offset=None):
        """(B, 3, H, W) frames in [-1, 1] -> (cropped faces (n, 3, face_h, face_w) in [-1, 1], affine matrices, indices of the
        frames with a face) or (None, None, None).  Detection runs on clamp((x + 1) / 2, 0, 1) * 255 like the reference."""
        if self.detector is not None:
            return self.detector.get_crop_face(bathed_imgs, only_keep_largest, only_center_face, resize, eye_dist_threshold,
                                               face_template_resize, face_template_x_offset, face_template_y_offset)
        from .retinaface_utils import estimate_affine_partial, get_center_face, get_largest_face
        face_template_resize = 1.0 if face_template_resize is None else face_template_resize
        face_template_x_offset = 0.0 if face_template_x_offset is None else face_template_x_offset
        face_template_y_offset = 0.0 if face_template_y_offset is None else face_template_y_offset
        if resize is not None:
            raise NotImplementedError("flair_amd: get_crop_face(resize=...) is not built (the reference multiplies a Python list "
                                      "by the float scale there, face_restoration_helper.py:152, which raises)")
        x = bathed_imgs.float().contiguous().to(self.device)
        B, _, H, W = x.shape
        # VF.normalize(x, [-1] * 3, [2] * 3).clamp(0, 1) * 255 = clamp(127.5 x + 127.5, 0, 255): folded into the detector's
        # mean-subtraction launch (`pre`)
        dets = self._detector().batched_detect_faces(x, 0.5, pre=(127.5, 127.5, 0.0, 255.0))
        # the reference zips the per-frame results with the frames, so a frame WITHOUT detections shifts the pairing
        # (retinaface.py:393-395 skips it); mirrored: results pair with frames in order
        affine_matrices, find_face_idx = [], []
        template = np.stack([self.face_template[:, 0] + face_template_x_offset,
                             self.face_template[:, 1] + face_template_y_offset], axis=1) * face_template_resize
        for idx, bboxes in enumerate(dets):
            landmarks, det_faces = [], []
            for bbox in bboxes:
                eye_dist = np.linalg.norm([bbox[5] - bbox[7], bbox[6] - bbox[8]])
                if eye_dist_threshold is not None and eye_dist < eye_dist_threshold:
                    continue
                n = 11 if self.template_3points else 15
                landmarks.append(np.array([[bbox[i], bbox[i + 1]] for i in range(5, n, 2)]))
                det_faces.append(bbox[0:5])
            if len(det_faces) == 0:
                continue
            if only_keep_largest:
                _, k = get_largest_face(det_faces, H, W)
                landmark = landmarks[k]
            elif only_center_face:
                _, k = get_center_face(det_faces, H, W)
                landmark = landmarks[k]
            else:
                landmark = landmarks[0]
            M = estimate_affine_partial(landmark, template)        # cv2.estimateAffinePartial2D(..., method=cv2.LMEDS)[0]
            affine_matrices.append(M)
            find_face_idx.append(idx)
        if len(affine_matrices) == 0:
            return None, None, None
        cropped = self.get_crop_face_from_affine_matrices(x[find_face_idx].contiguous(), affine_matrices)
        return cropped, affine_matrices, find_face_idx

    def get_face_matrices(self, bathed_imgs, eye_dist_threshold=None, max_faces=None, face_template_resize=None,
                          face_template_x_offset=None, face_template_y_offset=None):
        """The detection and alignment of get_crop_faces_all without its crop: (B, 3, H, W) frames in [-1, 1] -> (K affine
        matrices, face_frames: the frame of every face, non-decreasing); K = 0 gives ([], []).  For callers that cut
        something other than these f32 frames with the matrices (flair_amd.facescore cuts the written bytes)."""
        if self.detector is not None:
            raise NotImplementedError("flair_amd: get_crop_faces_all needs the package's own detector (face_det): an external "
                                      "detector= object returns faces without their frames")
        from .retinaface_utils import select_faces
        face_template_resize = 1.0 if face_template_resize is None else face_template_resize
        face_template_x_offset = 0.0 if face_template_x_offset is None else face_template_x_offset
        face_template_y_offset = 0.0 if face_template_y_offset is None else face_template_y_offset
        x = bathed_imgs.float().contiguous().to(self.device)
        B, _, H, W = x.shape
        dets = self._detector().batched_detect_faces(x, 0.5, pre=(127.5, 127.5, 0.0, 255.0), keep_empty=True)
        if len(dets) != B:
            raise RuntimeError(f"batched_detect_faces(keep_empty=True) returned {len(dets)} entries for {B} frames")
        template = np.stack([self.face_template[:, 0] + face_template_x_offset,
                             self.face_template[:, 1] + face_template_y_offset], axis=1) * face_template_resize
        return select_faces(dets, H, W, template, template_3points=self.template_3points,
                            eye_dist_threshold=eye_dist_threshold, max_faces=max_faces)

    def get_crop_faces_all(self, bathed_imgs, eye_dist_threshold=None, max_faces=None, face_template_resize=None,
                           face_template_x_offset=None, face_template_y_offset=None):
        """Every face of every frame (extension; the reference keeps one per frame): (B, 3, H, W) frames in [-1, 1] ->
        (cropped faces (K, 3, face_h, face_w) in [-1, 1] or None, K affine matrices, face_frames: the frame of every face,
        non-decreasing).  A frame may have no face or several (retinaface_utils.select_faces: largest first, at most
        ``max_faces`` per frame); K = 0 gives (None, [], [])."""
        x = bathed_imgs.float().contiguous().to(self.device)
        affine_matrices, face_frames = self.get_face_matrices(x, eye_dist_threshold, max_faces, face_template_resize,
                                                              face_template_x_offset, face_template_y_offset)
        if len(affine_matrices) == 0:
            return None, [], []
        return self.get_crop_face_from_affine_matrices(x, affine_matrices, face_frames), affine_matrices, face_frames

    def _consts(self, dev):
        c = self._const.get(dev)
        if c is None:
            c = (torch.tensor(self.mask_colormap, dtype=torch.float64, device=dev),
                 torch.from_numpy(gaussian_kernel(101, 26.0)).to(dev))
            self._const[dev] = c
        return c

    def _minv(self, mats, dev, twice=False):
        """The dst -> src matrices warpAffine derives from its argument (its inverse, in double): (N, 6) on the GPU.
        ``twice``: of the INVERSE matrices (inverse_faces warps with inverse_affine, which warpAffine inverts again).
        Cached per matrix list by content: the sampler passes the same list to three calls in every denoising step, and an
        upload from pageable host memory is a synchronous copy in the middle of the step."""
        arr = np.stack([np.asarray(m, dtype=np.float64).reshape(2, 3) for m in mats])
        key = (arr.tobytes(), str(dev), bool(twice))
        hit = self._minv_cache.get(key)
        if hit is None:
            src = [invert_affine(m) for m in arr] if twice else list(arr)
            hit = torch.from_numpy(np.stack([invert_affine(m).reshape(6) for m in src])).to(dev)
            if len(self._minv_cache) >= 64:
                self._minv_cache.clear()
            self._minv_cache[key] = hit
        return hit

    def _index(self, values, dev):
        """A host list of ints as an int32 device tensor, cached by content like _minv (same reason)."""
        key = (tuple(int(v) for v in values), str(dev))
        hit = self._index_cache.get(key)
        if hit is None:
            hit = torch.tensor(key[0], dtype=torch.int32).to(dev)
            if len(self._index_cache) >= 64:
                self._index_cache.clear()
            self._index_cache[key] = hit
        return hit

    @staticmethod
    def frame_starts(face_frames, T):
        """CSR form of a sorted face -> frame list: frame t owns faces starts[t] .. starts[t + 1] - 1."""
        frames = [int(f) for f in face_frames]
        if any(a > b for a, b in zip(frames, frames[1:])) or (frames and not 0 <= frames[0] <= frames[-1] < T):
            raise ValueError(f"face_frames must be non-decreasing with entries in [0, {T}) (got {frames})")
        starts, k = [0], 0
        for t in range(T):
            while k < len(frames) and frames[k] == t:
                k += 1
            starts.append(k)
        return starts

    def get_crop_face_from_affine_matrices(self, bathed_imgs, affine_matrices, face_frames=None):
        """(B, 3, H, W) in [-1, 1] -> (B, 3, face_h, face_w) in [-1, 1]: per frame
        ``cv2.warpAffine(clamp((x+1)/2, 0, 1)*255, M, face_size, INTER_CUBIC, BORDER_CONSTANT, (135, 133, 132))``,
        ``/ 255``, ``(y - 0.5) / 0.5``, clamp -- one launch for the batch.
        ``face_frames`` (extension): matrix k crops frame face_frames[k] -> (K, 3, face_h, face_w), read straight from
        the frames by flair_warp_affine_cubic_indexed (no gathered copy of them)."""
        if len(affine_matrices) == 0:
            return None
        x = bathed_imgs.float().contiguous()
        w, h = self.face_size
        if face_frames is not None:
            if len(face_frames) != len(affine_matrices):
                raise ValueError("one frame index per affine matrix is needed")
            return ops.warp_affine_cubic(x, self._minv(affine_matrices, x.device), (h, w), border=(135.0, 133.0, 132.0),
                                         pre=True, post=True, src_index=self._index(face_frames, x.device),
                                         src_index_host=face_frames)
        if len(affine_matrices) != x.shape[0]:
            raise ValueError("one affine matrix per frame is needed")
        return ops.warp_affine_cubic(x, self._minv(affine_matrices, x.device), (h, w), border=(135.0, 133.0, 132.0),
                                     pre=True, post=True)

    def get_inverse_affine(self, affine_matrices):
        return [invert_affine(m) for m in affine_matrices]

    def inverse_faces(self, restored_face_imgs, affine_matrices):
        """(B, 3, h, w) restored faces -> (faces warped back (B, 3, h, w) in [-1, 1], paste masks (B, 1, h, w) float32)."""
        if self.face_parse is None:
            raise RuntimeError("FaceRestoreHelper.inverse_faces needs face_parse=ParseNet(...) or BiSeNet(...) (facelib/parsing/)")
        x = restored_face_imgs.float().contiguous()
        B, _, h, w = x.shape
        lut, kern = self._consts(x.device)
        idx = self.face_parse.parse_indices(x)                                  # face_parse(x)[0].argmax(dim=1), (B, h, w) int32
        mask = ops.face_mask_blur(idx.reshape(-1), B, h, w, lut, kern, repeats=2, edge=10, div=255.0)
        # warpAffine(., inverse_affine) inverts its argument again: dst -> src = inv(inv(M)), rounded as OpenCV rounds it
        minv = self._minv(affine_matrices, x.device, twice=True)
        inv_faces = ops.warp_affine_cubic(x, minv, (h, w), pre=True, post=True)
        inv_masks = ops.warp_affine_cubic(mask, minv, (h, w))
        return inv_faces, inv_masks

    def paste_faces(self, x0, restored_faces, affine_matrices, face_frames):
        """inverse_faces and the blend of gaussian_diffusion.py:491 for any number of faces per frame (extension): the K
        restored faces ((K, 3, h, w) in [-1, 1], face k of frame face_frames[k], sorted by frame) are parsed and masked as
        in inverse_faces, then warped back and blended into x0 (T, 3, H, W) by one flair_face_paste launch, in list order
        (a later face of a frame lands on top of an earlier one).  Frames without a face come back as x0.  -> x_with_face."""
        if self.face_parse is None:
            raise RuntimeError("FaceRestoreHelper.paste_faces needs face_parse=ParseNet(...) or BiSeNet(...) (facelib/parsing/)")
        x0 = x0.float().contiguous()
        T = x0.shape[0]
        if len(face_frames) != len(affine_matrices):
            raise ValueError("one frame index per affine matrix is needed")
        starts = self.frame_starts(face_frames, T)
        dev = x0.device
        if len(affine_matrices) == 0:
            return ops.face_paste(x0, None, None, None, self._index(starts, dev), starts)
        x = restored_faces.float().contiguous()
        K, _, h, w = x.shape
        if K != len(affine_matrices):
            raise ValueError(f"{K} restored faces for {len(affine_matrices)} affine matrices")
        lut, kern = self._consts(dev)
        idx = self.face_parse.parse_indices(x)
        mask = ops.face_mask_blur(idx.reshape(-1), K, h, w, lut, kern, repeats=2, edge=10, div=255.0)
        minv = self._minv(affine_matrices, dev, twice=True)
        return ops.face_paste(x0, x, mask, minv, self._index(starts, dev), starts)
