"""Drop-in for the real-time demo's ``process()`` (reference nano_demo/core/__init__.py:35-80) with every step on the
device: BGR frame -> RGB -> centre square crop -> resize_align_multi_scale -> get_multi_stage_outputs /
aggregate_results -> fast_utils.group.HeatmapParser.parse_batch -> utils.vis.get_annotated_image.  Nothing here
synchronises: the caller's read of the returned image is the only wait."""
import numpy as np
import torch

from .core.inference import aggregate_results, get_multi_stage_outputs
from .fast_utils.group import HeatmapParser
from .utils.transforms import ToTensorNormalize, get_multi_scale_size, resize_align_multi_scale
from .utils.vis import get_annotated_image


def process(cfg, frame, executor, parser=None, dataset='CROWDPOSE', res=224, return_records=False):
    """``frame``: BGR uint8 [H,W,3], NumPy array or (host / device) tensor.  ``executor``: any callable that maps the
    normalised [1,3,Hd,Wd] float32 device tensor to the network's two output tensors.  ``parser``: a
    fast_utils.group.HeatmapParser to reuse (the reference builds one per frame).  Returns the annotated BGR crop, a uint8
    device tensor; with ``return_records`` also (ans [M,J,4], num [1] int32) on the device.  An image whose assignment
    hit the fast parser's round cap (num = -1) comes back un-annotated."""
    parser = HeatmapParser(cfg) if parser is None else parser
    if not isinstance(frame, torch.Tensor):
        frame = torch.from_numpy(np.ascontiguousarray(frame))
    if frame.dtype != torch.uint8 or frame.dim() != 3 or frame.shape[2] != 3:
        raise ValueError('frame must be HxWx3 uint8')
    image = frame.cuda().flip(2)                                     # cv2.COLOR_BGR2RGB
    h, w = int(image.shape[0]), int(image.shape[1])
    img_res = min(h, w)
    half = img_res // 2
    image = image[h // 2 - half:h // 2 + half, w // 2 - half:w // 2 + half].contiguous()
    scales = list(cfg.TEST.SCALE_FACTOR)
    get_multi_scale_size(image, cfg.DATASET.INPUT_SIZE, 1.0, min(scales))
    base_size = (res, res)
    transforms = ToTensorNormalize()
    with torch.no_grad():
        final_heatmaps, tags_list = None, []
        for s in sorted(scales, reverse=True):
            image_resized, _, _ = resize_align_multi_scale(image, cfg.DATASET.INPUT_SIZE, s, min(scales))
            x = transforms(image_resized)[None]
            _, heatmaps, tags = get_multi_stage_outputs(cfg, executor, x, cfg.TEST.FLIP_TEST, cfg.TEST.PROJECT2IMAGE,
                                                        base_size)
            final_heatmaps, tags_list = aggregate_results(cfg, s, final_heatmaps, tags_list, heatmaps, tags)
        final_heatmaps = final_heatmaps / float(len(scales))
        tags = torch.cat(tags_list, dim=4)
        ans, num = parser.parse_batch(final_heatmaps, tags, img_res / res)
        output = get_annotated_image(image, ans[0], dataset=dataset, count=num)
    return (output, ans[0], num) if return_records else output
