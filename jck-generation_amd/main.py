"""Entry point - drop-in for the reference's main.py: same flags (-t -pm -lf -m -w -b -e -mlr -milr -wd -snt), same global
seeding, same wiring (preprocessor -> Generator/Discriminator -> trainer -> train()).  Run from this directory:

    python main.py -m DCGAN -b 256 -e 1 -mlr 0.0002
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 main.py -m DCGAN -b 256   # data parallel

Note: the CLI default learning rate 0.1 is the reference's (main.py:54); it saturates the losses after one step - pass
-mlr 0.0002 for meaningful training.  `torch.autograd.set_detect_anomaly(True)` of the reference is not enabled: the native
step has no autograd graph to check."""
import argparse
import os
import random
from datetime import datetime

import numpy as np
import torch

from change_randomseed import RANDOMSEED
from enums import ModelEnum
from logger.main_logger import MainLogger


def seed_everything(seed=RANDOMSEED):
    random.seed(seed)
    os.environ["PYTHONHASHSEED"] = str(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed_all(seed)


def get_arg_parse(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("-t", "--test", type=int, default=0, help="test mode (unused, kept for compatibility)")
    p.add_argument("-pm", "--model_path", type=str, default="", help="model folder name")
    p.add_argument("-lf", "--log_file", type=int, default=1, help="write a log file: 0=false, 1=true")
    p.add_argument("-m", "--model", type=ModelEnum, choices=list(ModelEnum), default=ModelEnum.DCGAN, help="model to train")
    p.add_argument("-w", "--num_worker", type=int, default=0, help="DataLoader workers")
    p.add_argument("-b", "--batch_size", type=int, default=128, help="training batch size (per GPU)")
    p.add_argument("-e", "--epoch", type=int, default=100, help="epochs")
    p.add_argument("-mlr", "--max_learning_rate", type=float, default=0.1, help="Adam learning rate")
    p.add_argument("-milr", "--min_learning_rate", type=float, default=1e-4, help="unused, kept for compatibility")
    p.add_argument("-wd", "--weight_decay", type=float, default=5e-4, help="unused, kept for compatibility")
    p.add_argument("-snt", "--nesterov", type=int, default=1, help="unused, kept for compatibility")
    # not in the namespace unless given (default 0, read by the trainer): the reference's flag set stays as it is
    p.add_argument("-gpb", "--gp_backward", type=int, choices=(0, 1), default=argparse.SUPPRESS,
                   help="DCGAN: back-propagate the gradient penalty into D (1); 0 (default) = the reference, which only logs it")
    p.add_argument("--ema_decay", type=float, default=argparse.SUPPRESS,
                   help="keep an exponential moving average of G's weights with this decay (e.g. 0.999): evaluation samples it and "
                        "checkpoints gain 'model_g_ema'; absent or 0 = the reference, which has none")
    p.add_argument("--ema_start", type=int, default=argparse.SUPPRESS,
                   help="first optimiser step that averages; before it the average equals the weights (default 0)")
    p.add_argument("--extra_metrics", type=int, choices=(0, 1), default=argparse.SUPPRESS,
                   help="1: every evaluation also reports KID, improved precision / recall (CGAN: intra-KID too) on one more log "
                        "line and keeps 'kid' (CGAN: 'intra_kid') best checkpoints; absent or 0 = the reference's scores only")
    p.add_argument("--data", type=str, default=argparse.SUPPRESS, metavar="FILE.npz",
                   help="train on this dataset instead of CIFAR-100: `images` uint8 [N,H,W,3] (any H, W up to 1024; what generate.py "
                        "writes) and `labels` int [N] (CGAN: required, 0..99; DCGAN: optional).  Every image is resized to "
                        "image_size x image_size exactly as transforms.Resize((S, S)) would: a non-square source is squeezed unless "
                        "--crop is given")
    p.add_argument("--image_size", type=int, choices=(64, 128), default=argparse.SUPPRESS,
                   help="DCGAN: side of the generated and the training images; 128 builds the nets with one more stride-2 stage "
                        "(absent = 64, the reference)")
    p.add_argument("--mirror", type=int, choices=(0, 1), default=argparse.SUPPRESS,
                   help="1: mirror every training image left-right with probability 1/2, drawn anew each epoch (needs the "
                        "device-resident input pipeline); absent or 0 = the reference, which has no augmentation")
    p.add_argument("--crop", type=str, choices=("center", "random"), default=argparse.SUPPRESS,
                   help="resize a square box of every training image instead of the whole image (CenterCrop / RandomCrop in front of "
                        "the Resize): center = the centred box; random = a box drawn anew per image and epoch (needs the "
                        "device-resident input pipeline).  Evaluation reads the centred box in both modes")
    p.add_argument("--crop_size", type=int, default=argparse.SUPPRESS, metavar="K",
                   help="side of the --crop box in source pixels, 1..min(H, W) (absent = min(H, W), the largest centred square)")
    args = p.parse_args(argv)
    if hasattr(args, "crop_size") and not hasattr(args, "crop"):
        p.error("--crop_size K needs --crop center or --crop random")
    if getattr(args, "image_size", 64) != 64 and args.model != ModelEnum.DCGAN:
        p.error("--image_size 128: the 128x128 topology exists for DCGAN only (CGAN's Linear(8392,256) fixes 64x64)")
    return args


def main(args: argparse.Namespace):
    datetime_now = args.model_path if args.model_path != "" else datetime.now().strftime("%Y%m%d_%H%M%S")
    args.save_path = os.path.join(".", "save", str(args.model).lower(), datetime_now)
    os.makedirs(args.save_path, exist_ok=True)

    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world > 1 and not torch.distributed.is_initialized():
        local = int(os.environ.get("LOCAL_RANK", "0"))
        torch.cuda.set_device(local)
        torch.distributed.init_process_group("nccl", device_id=torch.device("cuda", local))   # "nccl" is RCCL on ROCm

    logger = MainLogger(args)
    logger.debug(f"args: {vars(args)}")
    logger.debug("init data preprocessing")

    if args.model == ModelEnum.DCGAN:
        from model import DCGAN
        from preprocess.dcgan_data_preprocessor import DCGANDataPreprocessor
        from train.dcgan_trainer import DCGANTrainer
        data_pre = DCGANDataPreprocessor(args)
        data_pre.transform_data()
        size = {"image_size": args.image_size} if getattr(args, "image_size", 64) != 64 else {}
        trainer = DCGANTrainer(args, DCGAN.Generator(**size), DCGAN.Discriminator(**size), data_pre)
    else:
        from model import CGAN
        from preprocess.cgan_data_preprocessor import CGANDataPreprocessor
        from train.cgan_trainer import CGANTrainer
        data_pre = CGANDataPreprocessor(args)
        data_pre.transform_data()
        trainer = CGANTrainer(args, CGAN.Generator(), CGAN.Discriminator(), data_pre)
    trainer.train()
    if world > 1:
        torch.distributed.destroy_process_group()


seed_everything()

if __name__ == "__main__":
    main(get_arg_parse())
