"""Bayesian YOLOv3 (MC dropout, aleatoric loss), resumed from the pretraining run and trained on TFRecord shards.

Run:  python uncertainty_training.py

Counterpart of the reference script of the same name: the config below carries its keys and default values; edit the paths and
sizes for your data.  lib_yolo.train.run does the rest: a log file under log_path, then the detection heads are trained on the
device with the Darknet-53 backbone frozen, from shards cropped and augmented on the GPU.  The optional key 'seed' (default 0)
fixes the feed's draws and the dropout stream.
"""
import os

from lib_yolo import train, yolov3


def main():
    config = {
        'training': True,  # False: the qualitative viewer (not provided here)
        'resume_training': True,  # continue from resume_checkpoint
        'resume_checkpoint': './checkpoints/pretraining/pretraining-125000',  # a checkpoint prefix, or 'last' of checkpoint_path/run_id
        'priors': yolov3.ECP_9_PRIORS,  # anchor boxes; replace for another dataset
        'run_id': 'epi_ale',  # names the log file and the checkpoint folder
        'checkpoint_path': './checkpoints',
        'tensorboard_path': './tensorboard',
        'log_path': './log',
        'ckp_max_to_keep': 75,
        'checkpoint_interval': 5000,
        'ign_thresh': 0.7,
        'crop_img_size': [768, 1440, 3],
        'full_img_size': [1024, 1920, 3],  # size of the frames in the shards
        'train_steps': 500000,
        'darknet53_weights': './darknet53.conv.74',  # Darknet .weights of the backbone
        'batch_size': 2,  # images per step
        'lr': 1e-5,
        'cpu_thread_cnt': 24,  # host threads decoding PNGs
        'crop': True,  # train on random crops (and rescaled crops)
        'freeze_darknet53': True,  # only True is supported: the heads are trained
        'inference_mode': False,
        'aleatoric_loss': True,
        'cls_cnt': 2,  # classes in the shards
        'implicit_background_class': True,  # True: labels in the shards start at 1 (TF object detection API), False: at 0
        'train': {
            'file_pattern': os.path.expandvars('$HOME/data/ecp/tfrecords/ecp-day-train-*-of-*'),  # your training shards
            'num_shards': 20,
            'shuffle_buffer_size': 2000,
            'cache': False,  # True: hold every record in host memory after the first epoch
        },
        'val': {
            'file_pattern': os.path.expandvars('$HOME/data/ecp/tfrecords/ecp-day-val-*-of-*'),  # your validation shards
            'num_shards': 4,
            'shuffle_buffer_size': 10,
            'cache': False,  # as for train
        },
    }
    train.run(yolov3.bayesian_yolov3_aleatoric, config)


if __name__ == '__main__':
    train.console_logging()
    main()
