"""Training-side helpers of the reference's `lib_yolo/utils.py`: `add_file_logging` (the run's log file next to the console
output) and `qualitative_eval`, which this build does not provide (it is an interactive matplotlib viewer)."""
import logging
import os

LOG_FORMAT = '%(asctime)s, %(levelname)-8s %(message)s'
LOG_DATEFMT = '%a, %d %b %Y %H:%M:%S'


def add_file_logging(config, override_existing=False):
    """Send INFO and above of the root logger to <log_path>/<run_id>.log as well.  An existing file of that name is an error
    unless override_existing (it is then truncated).  Returns the handler (remove it from the root logger to stop)."""
    log_dir = config['log_path']
    target = os.path.join(log_dir, config['run_id'] + '.log')
    os.makedirs(log_dir, exist_ok=True)
    if not override_existing and os.path.exists(target):
        raise RuntimeError('Logging file {} already exists'.format(target))
    handler = logging.FileHandler(target, mode='w')
    handler.setLevel(logging.INFO)
    handler.setFormatter(logging.Formatter(fmt=LOG_FORMAT, datefmt=LOG_DATEFMT))
    logging.getLogger().addHandler(handler)
    return handler


def qualitative_eval(model_cls, config):
    raise NotImplementedError("'training': False runs the reference's qualitative_eval, an interactive viewer of a checkpoint's "
                              "detections; it is not part of this build -- run the inference scripts on the checkpoint instead")
